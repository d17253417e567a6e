"""CPU tests of the tiled scan path: the four properties of the tile grid over random draws, its edge
cases and refusals, host_tiles against the mask written out, host_merge on hand-made arenas, a
host-only TileStore under ScanLoader.host_batch, and the new flags of tools/detect.py."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, load_pkg
from scan_tile_cases import OVERLAP, TILE, edge_clouds, hand_made_tiles

load_pkg()
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
ST = importlib.import_module("3dioumatch_amd.votenet.scan_tiles")
D = importlib.import_module("3dioumatch_amd.votenet.detect")
V = importlib.import_module("3dioumatch_amd.votenet")

INF = np.float32(np.inf)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the grid
def _draws(count, seed):
    """(lo, hi, t, overlap) with hi - lo from well below t to forty tiles, overlap <= t / 2"""
    g = np.random.default_rng(seed)
    for i in range(count):
        t = float(np.exp(g.uniform(np.log(0.5), np.log(20.0))))
        L = t * float(np.exp(g.uniform(np.log(0.3), np.log(40.0))))
        lo = float(np.float32(g.uniform(-100, 100)))
        hi = float(np.float32(lo + L))
        overlap = (0.0, t / 2)[i % 2] if i % 10 < 2 else float(g.uniform(0, t / 2))
        yield lo, hi, t, overlap


def _probe(g, lo, hi, bounds):
    """float32 coordinates of the axis: random ones, the extent's ends, and every finite bound with
    its two float32 neighbours"""
    finite = bounds[np.isfinite(bounds)].astype(np.float32)
    pts = [g.uniform(lo, hi, 64).astype(np.float32), np.array([lo, hi], np.float32), finite,
           np.nextafter(finite, -INF), np.nextafter(finite, INF)]
    return np.concatenate(pts)


def test_grid_properties_over_random_draws():
    g = np.random.default_rng(1)
    many = 0
    for lo, hi, t, overlap in _draws(3000, 7):
        wlo, whi, clo, chi = ST.axis_windows(lo, hi, t, overlap)
        n = len(wlo)
        assert wlo.dtype == whi.dtype == clo.dtype == chi.dtype == np.float32
        assert len(whi) == len(clo) == len(chi) == n
        many += n > 1
        x = _probe(g, lo, hi, np.concatenate([wlo, whi, clo, chi]))
        in_core = (clo[:, None] <= x[None]) & (x[None] < chi[:, None])
        in_window = (wlo[:, None] <= x[None]) & (x[None] < whi[:, None])
        # the cores partition the axis: every float32 coordinate is in exactly one
        assert (in_core.sum(0) == 1).all(), (lo, hi, t, overlap)
        assert np.array_equal(clo[1:], chi[:-1]) and clo[0] == -INF and chi[-1] == INF
        # the owner's window contains the point
        assert in_window[in_core].all(), (lo, hi, t, overlap)
        # at most three windows hold a point
        assert in_window.sum(0).max() <= 3, (lo, hi, t, overlap)
        # every cut lies overlap / 2 inside both windows it separates, less four float32 ulps of the larger bound
        for i in range(n - 1):
            cut = np.float64(chi[i])
            slack = 4 * np.float64(np.spacing(np.float32(max(abs(whi[i]), abs(wlo[i + 1]), abs(chi[i])))))
            assert np.float64(whi[i]) - cut >= overlap / 2 - slack, (lo, hi, t, overlap, i)
            assert cut - np.float64(wlo[i + 1]) >= overlap / 2 - slack, (lo, hi, t, overlap, i)
        if n > 1:  # spread evenly, the last window ends at max, the effective overlap >= the nominal
            assert n == int(np.ceil((hi - lo - overlap) / (t - overlap)))
            assert wlo[0] == -INF and whi[-1] == INF
    assert many > 1500  # most draws are scans larger than a tile


def test_tiles_are_products_of_the_axes_row_major():
    bounds = np.array([[0, 10, -3, 2], [5, 6, 0, 30]], np.float32)
    grid = ST.tile_grid(bounds, (4.0, 3.0), 1.0)
    assert grid["shape"].tolist() == [[2, 3], [15, 1]]  # ny, nx
    assert grid["tiles"].tolist() == [6, 15] and grid["first"].tolist() == [0, 6]
    assert grid["parent"].tolist() == [0] * 6 + [1] * 15
    assert grid["iy"][:6].tolist() == [0, 0, 0, 1, 1, 1] and grid["ix"][:6].tolist() == [0, 1, 2, 0, 1, 2]
    xw = ST.axis_windows(0, 10, 4.0, 1.0)
    yw = ST.axis_windows(-3, 2, 3.0, 1.0)
    for t in range(6):
        iy, ix = divmod(t, 3)
        assert grid["window"][t].tolist() == [xw[0][ix], xw[1][ix], yw[0][iy], yw[1][iy]]
        assert grid["core"][t].tolist() == [xw[2][ix], xw[3][ix], yw[2][iy], yw[3][iy]]
    assert grid["window"].dtype == grid["core"].dtype == np.float32
    # x of [0, 10] in tiles of 4 with overlap 1: starts 0, 3, 6, cuts in the middle of the overlaps
    assert xw[0].tolist() == [-INF, 3, 6] and xw[1].tolist() == [4, 7, INF]
    assert xw[2].tolist() == [-INF, 3.5, 6.5] and xw[3].tolist() == [3.5, 6.5, INF]
    assert ST.tile_grid(bounds, 4.0, 1.0)["shape"].tolist() == [[2, 3], [10, 1]]  # one size: both axes


def test_an_extent_within_the_tile_is_one_infinite_window_and_just_above_it_two():
    for L in (0.0, 1.0, 5.0):
        for w in ST.axis_windows(2.0, 2.0 + L, 5.0, 1.0):
            assert w.shape == (1,) and np.isinf(w[0])
    grid = ST.tile_grid(np.array([[2, 7, -1, 1]], np.float32), (5.0, 5.0), 1.0)
    assert grid["tiles"].tolist() == [1]
    assert grid["window"].tolist() == [[-INF, INF, -INF, INF]] and grid["core"].tolist() == [[-INF, INF, -INF, INF]]
    hi = float(np.nextafter(np.float32(7), INF))
    wlo, whi, clo, chi = ST.axis_windows(2.0, hi, 5.0, 1.0)
    assert len(wlo) == 2 and wlo[0] == -INF and whi[1] == INF
    assert whi[0] == np.float32(7) and wlo[1] == np.float32(hi - 5.0)
    assert clo.tolist() == [-INF, chi[0]] and chi[1] == INF and wlo[1] < chi[0] < whi[0]


def test_grid_refusals():
    b = np.array([[0, 10, 0, 10]], np.float32)
    for overlap in (-0.1, 2.01, np.nan):
        with pytest.raises(ValueError, match="overlap"):
            ST.tile_grid(b, (4.0, 6.0), overlap)
    ST.tile_grid(b, (4.0, 6.0), 2.0)  # min(tile) / 2: allowed
    for tile in (0.0, (4.0, -1.0), (4.0, 0.0), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="tile"):
            ST.tile_grid(b, tile, 0.0)
    big = np.array([[0, 1, 0, 1], [0, 65.5, 0, 64.5]], np.float32)
    with pytest.raises(ValueError, match="scan wide: 65 x 66 tiles") as e:
        ST.tile_grid(big, 1.0, 0.0, names=["narrow", "wide"])
    assert "4096" in str(e.value)
    assert ST.tile_grid(np.array([[0, 64, 0, 64]], np.float32), 1.0, 0.0)["tiles"].tolist() == [4096]
    with pytest.raises(ValueError):
        ST.TileStore.from_store(SC.ScanStore([np.zeros((4, 3), np.float32)], None), 4.0, overlap=3.0)
    with pytest.raises(TypeError):
        ST.TileStore()


# ------------------------------------------------------------------ host_tiles against the mask
def _mask_by_hand(cloud, w):
    x, y = cloud[:, 0], cloud[:, 1]
    return (w[0] <= x) & (x < w[1]) & (w[2] <= y) & (y < w[3])


@pytest.mark.parametrize("columns", [6, 3])
def test_host_tiles_is_the_mask(columns):
    clouds = edge_clouds(columns)
    grid = ST.tile_grid(ST.host_bounds(clouds), TILE, OVERLAP)
    assert grid["tiles"].tolist() == [6, 3, 1]
    built, crops = ST.host_tiles(clouds, grid)
    assert built.tolist() == [0, 1, 2, 3, 4, 5, 6, 8, 9]  # tile 7, the empty one, is dropped
    for t, crop in zip(built, crops):
        p, w = grid["parent"][t], grid["window"][t]
        want = clouds[p][_mask_by_hand(clouds[p], w)]
        assert crop.shape == want.shape and np.array_equal(bits(crop), bits(want))
        for lo, hi, col in ((w[0], w[1], 0), (w[2], w[3], 1)) if p == 0 else ():  # scan 0 has the points on bounds
            if np.isfinite(lo):  # points exactly on a lower bound are in
                assert (clouds[p][:, col] == lo).sum() >= 20 and (crop[:, col] == lo).sum() >= 1
            if np.isfinite(hi):  # exactly on an upper bound: out
                assert (clouds[p][:, col] == hi).sum() >= 20 and not (crop[:, col] == hi).any()
    assert crops[7].shape[0] == 1 and crops[7][0, 0] == np.float32(9.75)  # the one-point tile
    assert np.array_equal(bits(crops[8]), bits(clouds[2]))  # a scan within one tile: its own rows
    # every point of a scan is in a tile that owns it
    for s, cloud in enumerate(clouds):
        owners = np.zeros(len(cloud), int)
        for t in range(grid["first"][s], grid["first"][s] + grid["tiles"][s]):
            own = ST.in_box(cloud, grid["core"][t])
            assert not (own & ~ST.in_box(cloud, grid["window"][t])).any()
            owners += own
        assert (owners == 1).all()


def test_min_points_drops_small_tiles_and_leaves_one_per_scan():
    clouds = edge_clouds()
    grid = ST.tile_grid(ST.host_bounds(clouds), TILE, OVERLAP)
    counts = [int(_mask_by_hand(clouds[p], w).sum()) for p, w in zip(grid["parent"], grid["window"])]
    built, crops = ST.host_tiles(clouds, grid, min_points=2)
    assert built.tolist() == [0, 1, 2, 3, 4, 5, 6, 9]  # the one-point tile goes too
    built, crops = ST.host_tiles(clouds, grid, min_points=10 ** 6)  # nothing reaches it: the largest of each scan
    assert built.tolist() == [int(np.argmax(counts[:6])), 6, 9]
    assert [c.shape[0] for c in crops] == [max(counts[:6]), counts[6], 700]
    assert ST.host_tiles(clouds, grid, min_points=0)[0].tolist() == ST.host_tiles(clouds, grid)[0].tolist()


def test_a_host_only_tile_store_feeds_the_loader():
    clouds = edge_clouds()
    parent = SC.ScanStore(clouds, None, "scannet", names=["a", "b", "c"])
    store = ST.TileStore.from_store(parent, TILE, overlap=OVERLAP)
    assert isinstance(store, SC.ScanStore) and store.dev is None and store.device is None
    assert len(store) == 9 and store.parent.tolist() == [0] * 6 + [1, 1, 2]
    assert store.first.tolist() == [0, 6, 8] and store.tiles.tolist() == [6, 2, 1]
    assert store.names[:4] == ["a_tile00_00", "a_tile00_01", "a_tile00_02", "a_tile01_00"]
    assert store.names[6:] == ["b_tile00_00", "b_tile00_02", "c_tile00_00"]
    assert store.parent_names == ["a", "b", "c"] and store.columns == 6 and store.dataset == "scannet"
    assert store.window.shape == store.core.shape == (9, 4) and store.window.dtype == np.float32
    assert store.count.tolist() == [c.shape[0] for c in store.clouds]
    assert store.offset.tolist() == np.concatenate([[0], np.cumsum(store.count)[:-1]]).tolist()
    plain = SC.ScanStore(store.clouds, None, "scannet", names=store.names)
    assert np.array_equal(store.floor, plain.floor) and store.floor.dtype == np.float32
    for use_color in (False, True):
        got = SC.ScanLoader(store, 64, use_color=use_color, seed=3).host_batch([0, 7, 8, 4], counter=2)
        want = SC.ScanLoader(plain, 64, use_color=use_color, seed=3).host_batch([0, 7, 8, 4], counter=2)
        assert np.array_equal(bits(got["point_clouds"]), bits(want["point_clouds"]))
        assert np.array_equal(got["scan_idx"], want["scan_idx"])
    assert (got["point_clouds"][1, :, 0] == np.float32(9.75)).all()  # the one-point tile, drawn 64 times
    small = ST.TileStore.from_store(parent, TILE, overlap=OVERLAP, min_points=10 ** 6)
    assert small.tiles.tolist() == [1, 1, 1] and len(small) == 3
    with pytest.raises(ValueError, match="ScanStore"):
        ST.TileStore.from_store(store, TILE)


# ------------------------------------------------------------------ host_merge on hand-made arenas
@pytest.mark.parametrize("NC", [0, 3])
def test_host_merge_on_hand_made_arenas(NC):
    planes, first, tiles, core, want_rows = hand_made_tiles(NC)
    K = 6
    out = D.host_merge(planes, first, tiles, core)
    cap = 4 * K
    assert out["count"].tolist() == [7, 5] and out["count"].dtype == np.int32
    assert out["tile"].shape == (2, cap) and out["box"].shape == (2, cap, 7) and out["corners"].shape == (2, cap, 8, 3)
    assert out["score"].shape == ((2, cap, NC) if NC else (2, cap))
    for s, rows in enumerate(want_rows):
        assert out["tile"][s, :len(rows)].tolist() == [t for t, _ in rows]
        for i, (t, r) in enumerate(rows):
            for name in ("proposal", "cls", "score", "box", "corners"):
                assert np.array_equal(out[name][s, i], planes[name][t, r]), (name, s, i)
        for name in ("tile", "proposal", "cls", "score", "box", "corners"):
            assert not out[name][s, len(rows):].any(), name  # rows past count: zero
    wide = D.host_merge(planes, first, tiles, core, cap=cap + 5)
    assert wide["tile"].shape == (2, cap + 5) and wide["count"].tolist() == [7, 5]

    # the merged layout read back through TiledDetections, from a host arena
    layout, words = D.merged_layout(2, cap, NC)
    arena = np.zeros(words, np.float32)
    for name, (at, shape) in layout.items():
        flat = np.ascontiguousarray(out[name]).reshape(-1)
        arena[at:at + flat.size] = flat.view(np.float32) if flat.dtype == np.int32 else flat

    class Store(object):
        parent_names = ["big", "room"]
        names = ["big_tile%02d_%02d" % divmod(t, 2) for t in range(4)] + ["room_tile00_00"]
        window = core  # (stand-ins: save() writes them out)

    Store.first, Store.tiles, Store.core = first, tiles, core
    found = D.TiledDetections(arena, Store, cap, K, NC, 3)
    assert isinstance(found, D.Detections) and len(found) == 2 and found.names == ["big", "room"]
    assert found.by_name("room")["count"] == 5 and found[0]["tile"].dtype == np.int32
    for name in D.MERGED_PLANES:
        assert np.array_equal(found.planes()[name], out[name]), name
    listing = found.as_map_cls()
    for s, rows in enumerate(want_rows):
        order = sorted(rows, key=lambda tr: (tr[0], planes["proposal"][tr]))  # tile, then proposal
        if NC:
            want = [(ii, planes["corners"][tr], planes["score"][tr][ii]) for ii in range(3) for tr in order]
        else:
            want = [(int(planes["cls"][tr]), planes["corners"][tr], planes["score"][tr]) for tr in order]
        assert len(listing[s]) == len(want)
        for (gc, gb, gs), (wc, wb, ws) in zip(listing[s], want):
            assert gc == wc and np.array_equal(bits(gb), bits(wb)) and bits(gs) == bits(ws)


def test_tiled_detections_save(tmp_path):
    planes, first, tiles, core, want_rows = hand_made_tiles(3)
    out = D.host_merge(planes, first, tiles, core)
    layout, words = D.merged_layout(2, 24, 3)
    arena = np.zeros(words, np.float32)
    for name, (at, shape) in layout.items():
        flat = np.ascontiguousarray(out[name]).reshape(-1)
        arena[at:at + flat.size] = flat.view(np.float32) if flat.dtype == np.int32 else flat

    class Store(object):
        parent_names = ["big", "room"]
        names = ["t%d" % t for t in range(5)]

    Store.first, Store.tiles, Store.core, Store.window = first, tiles, core, core + 1
    D.TiledDetections(arena, Store, 24, 6, 3, 3).save(str(tmp_path / "out"))
    with np.load(str(tmp_path / "out" / "big.npz")) as f:
        assert int(f["count"]) == 7 and f["tile"].tolist() == [1, 1, 1, 2, 2, 2, 2] and f["box"].shape == (7, 7)
        assert f["window"].shape == (4, 4) and np.array_equal(f["core"], core[:4]) and int(f["tile_first"]) == 0
        assert f["tile_names"].tolist() == ["t0", "t1", "t2", "t3"]
    with np.load(str(tmp_path / "out" / "room.npz")) as f:
        assert int(f["count"]) == 5 and int(f["tile_first"]) == 4 and f["window"].shape == (1, 4)


def test_exports():
    assert V.detect_tiled is D.detect_tiled and V.TiledDetections is D.TiledDetections
    assert V.TileStore is ST.TileStore and V.tile_grid is ST.tile_grid
    L = importlib.import_module("3dioumatch_amd._lib")
    for name in ("scene_scan_bounds", "scene_scan_tile_count", "scene_scan_tile_gather", "scene_detections_merge"):
        assert name in L._LOADER_SIGNATURES and name not in L.EXPORTS and hasattr(L.lib, name)
    with pytest.raises(ValueError, match="TileStore"):
        V.detect_tiled(None, SC.ScanStore([np.zeros((4, 3), np.float32)], None), {})


# ------------------------------------------------------------------ tools/detect.py
def _tool():
    spec = importlib.util.spec_from_file_location("tools_detect_tiled", os.path.join(ROOT, "tools", "detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_detect_tool_tiling_flags():
    tool = _tool()
    flags = tool.parser().parse_args(["a.npy"])
    assert flags.tile is None and tool.tiling(flags) is None  # no --tile: the path as it was
    assert tool.tiling(tool.parser().parse_args(["a.npy", "--overlap", "2", "--min_points", "9"])) is None
    flags = tool.parser().parse_args(["a.npy", "--tile", "8"])
    assert tool.tiling(flags) == ((8.0, 8.0), 1.0, 1)
    flags = tool.parser().parse_args(["--tile", "8", "6.5", "--overlap", "0.5", "--min_points", "2000", "--", "a.npy"])
    assert tool.tiling(flags) == ((8.0, 6.5), 0.5, 2000)
    with pytest.raises(SystemExit, match="TX"):
        tool.tiling(tool.parser().parse_args(["--tile", "8", "6", "4"]))
