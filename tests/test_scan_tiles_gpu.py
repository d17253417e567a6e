"""The tiled scan path on the MI355X: scene_scan_bounds against numpy, TileStore's crops against
host_tiles (bit for bit, across a segment boundary too) and their floors against host_floor, the
batches of ScanLoader over a TileStore against those of a plain ScanStore of the host crops,
scene_detections_merge against host_merge, detect_tiled() end to end -- equal to detect() where every
scan fits one tile, equal to host_merge of detect() on the tiles where it does not, reproducible and
without a synchronising call -- and the four bindings on poisoned allocations."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import dirty_memory
from conftest import load_pkg
from scan_tile_cases import OVERLAP, TILE, edge_clouds, hand_made_tiles

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.scan_data"),
            importlib.import_module("3dioumatch_amd.votenet.scan_tiles"),
            importlib.import_module("3dioumatch_amd.votenet.detect"))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_floor(got, want):
    got, want = np.float32(got), np.float32(want)
    return got == want and (got.tobytes() == want.tobytes() or got == 0)


# ------------------------------------------------------------------ scene_scan_bounds
# one row under, at and over a wave, the workgroup (1024) and the segment (65536), and two segments and a bit
BOUNDS_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 65535, 65536, 65537, 131073)


@pytest.mark.parametrize("columns", [3, 6])
def test_bounds_are_numpy_min_and_max(columns):
    _, SC, ST, _ = _mods()
    assert (ST.BLOCK, ST.SEGMENT) == (1024, 65536)
    g = np.random.default_rng(5)
    clouds = []
    for i, n in enumerate(BOUNDS_SIZES):
        c = ((g.random((n, columns)) - 0.3) * (i + 1)).astype(np.float32)
        c[n - 1, 0], c[n - 1, 1] = -50 - i, 70 + i  # the extremes in the scan's last row ...
        if n > 1:
            c[0, 0], c[0, 1] = 40 + i, -60 - i      # ... and its first
        clouds.append(c)
    store = SC.ScanStore(clouds, DEV, "scannet")  # several scans in one store
    d = store.dev
    got = ST.scan_bounds_gpu(d["cloud"], d["offset"], d["count"], ST._segments(store.count))
    assert got.shape == (len(clouds), 4) and got.dtype == torch.float32
    got = got.cpu().numpy()
    want = ST.host_bounds(clouds)
    for i, n in enumerate(BOUNDS_SIZES):
        assert (got[i] == want[i]).all(), (n, got[i], want[i])
    assert got[0].tolist() == [-50, -50, 70, 70]


# ------------------------------------------------------------------ the crops
def _assert_store_is_host_tiles(ST, SC, store, clouds, tile, overlap, min_points=1):
    grid = ST.tile_grid(ST.host_bounds(clouds), tile, overlap)
    built, crops = ST.host_tiles(clouds, grid, min_points)
    assert len(store) == len(built)
    assert np.array_equal(store.parent, grid["parent"][built])
    assert np.array_equal(bits(store.window), bits(grid["window"][built]))
    assert np.array_equal(bits(store.core), bits(grid["core"][built]))
    assert store.count.dtype == np.int32 and store.count.tolist() == [c.shape[0] for c in crops]
    assert store.offset.tolist() == np.concatenate([[0], np.cumsum(store.count, dtype=np.int64)[:-1]]).tolist()
    flat = store.dev["cloud"].cpu().numpy()
    assert flat.shape == (int(store.count.sum()), clouds[0].shape[1])
    assert np.array_equal(bits(flat), bits(np.concatenate(crops)))
    assert np.array_equal(store.dev["count"].cpu().numpy(), store.count)
    assert np.array_equal(store.dev["offset"].cpu().numpy(), store.offset)
    for k in ("parent", "first", "tiles"):
        assert np.array_equal(store.dev[k].cpu().numpy(), getattr(store, k)), k
    for k in ("window", "core"):
        assert np.array_equal(bits(store.dev[k].cpu().numpy()), bits(getattr(store, k))), k
    floor = store.dev["floor"].cpu().numpy()
    for t, crop in enumerate(crops):
        assert same_floor(floor[t], SC.host_floor(crop[:, 2])), t
        assert np.array_equal(bits(store.clouds[t]), bits(crop))  # the lazy host rows
    assert np.array_equal(bits(store.floor), bits(floor))
    return built, crops


@pytest.mark.parametrize("columns", [6, 3])
@pytest.mark.parametrize("min_points", [1, 2, 10 ** 6])
def test_crops_are_host_tiles(columns, min_points):
    _, SC, ST, _ = _mods()
    clouds = edge_clouds(columns)
    parent = SC.ScanStore(clouds, DEV, "scannet", names=["a", "b", "c"])
    store = ST.TileStore.from_store(parent, TILE, overlap=OVERLAP, min_points=min_points)
    built, crops = _assert_store_is_host_tiles(ST, SC, store, clouds, TILE, OVERLAP, min_points)
    assert len(store) == {1: 9, 2: 8, 10 ** 6: 3}[min_points]
    assert isinstance(store, SC.ScanStore) and store.device == DEV and store.parent_names == ["a", "b", "c"]
    if min_points == 1:
        assert store.names[6:] == ["b_tile00_00", "b_tile00_02", "c_tile00_00"]  # b's middle tile is empty
        assert store.count[7] == 1                                                # the one-point tile
        assert np.array_equal(bits(crops[8]), bits(clouds[2]))                    # a scan within one tile: its rows


def test_crops_across_a_segment_boundary():
    _, SC, ST, _ = _mods()
    g = np.random.default_rng(21)
    n = 70001
    big = (g.random((n, 3)) * [12, 8, 3]).astype(np.float32)
    big[0, :2], big[1, :2] = (0, 0), (12, 8)
    clouds = [big, (g.random((300, 3)) * [3, 3, 3]).astype(np.float32)]
    parent = SC.ScanStore(clouds, DEV, "scannet")
    tile, overlap = (5.0, 5.0), 1.0  # 12 m x 8 m: 3 x 2 tiles
    store = ST.TileStore.from_store(parent, tile, overlap=overlap)
    assert store.tiles.tolist() == [6, 1]
    _assert_store_is_host_tiles(ST, SC, store, clouds, tile, overlap)
    # every tile of the big scan has rows on both sides of row 65536 of its parent
    for t in range(6):
        rows = np.nonzero(ST.in_box(big, store.window[t]))[0]
        assert rows[0] < ST.SEGMENT <= rows[-1], t


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("use_color", [False, True])
def test_batches_of_a_tile_store_are_those_of_a_store_of_the_crops(use_color):
    _, SC, ST, _ = _mods()
    clouds = edge_clouds(6)
    store = ST.TileStore.from_store(SC.ScanStore(clouds, DEV, "scannet"), TILE, overlap=OVERLAP)
    grid = ST.tile_grid(ST.host_bounds(clouds), TILE, OVERLAP)
    plain = SC.ScanStore(ST.host_tiles(clouds, grid)[1], DEV, "scannet", names=store.names)
    N = 512  # above, below and far above the tiles' counts
    a = SC.ScanLoader(store, N, use_color=use_color, seed=5)
    b = SC.ScanLoader(plain, N, use_color=use_color, seed=5)
    for ids, counter in ((np.arange(9), 0), ([7, 2, 8], 11)):
        got, want = a.batch(ids, counter), b.batch(ids, counter)
        assert torch.equal(got["point_clouds"].view(torch.int32), want["point_clouds"].view(torch.int32))
        assert torch.equal(got["scan_idx"], want["scan_idx"])
        host = a.host_batch(ids, counter)["point_clouds"]
        zero_floor = (store.floor[np.asarray(ids)] == 0).any()
        if not zero_floor:  # (the sign of a zero floor is unspecified)
            assert np.array_equal(bits(got["point_clouds"].cpu().numpy()), bits(host))


# ------------------------------------------------------------------ scene_detections_merge
def _arena_of(D, planes, layout_fn, *dims):
    layout, words = layout_fn(*dims)
    arena = np.zeros(words, np.float32)
    for name, (at, shape) in layout.items():
        flat = np.ascontiguousarray(planes[name]).reshape(-1)
        arena[at:at + flat.size] = flat.view(np.float32) if flat.dtype == np.int32 else flat
    return torch.from_numpy(arena).to(DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("NC", [0, 3])
def test_merge_is_host_merge(NC):
    _, _, _, D = _mods()
    planes, first, tiles, core, want_rows = hand_made_tiles(NC)
    T, K = planes["proposal"].shape
    S, cap = 2, 4 * K + 3  # three rows more than the scans' tiles can fill
    want = D.host_merge(planes, first, tiles, core, cap=cap)
    assert want["count"].tolist() == [len(r) for r in want_rows] == [7, 5]
    tile_arena = _arena_of(D, planes, D.arena_layout, T, K, NC)
    layout, words = D.merged_layout(S, cap, NC)
    sentinel = np.float32(7).view(np.uint32)

    def assert_planes(host, scans):
        for name, (at, shape) in layout.items():
            got = host[at:at + int(np.prod(shape))].reshape(shape).view(np.uint32)
            ref = np.ascontiguousarray(want[name]).view(np.uint32)
            for s_ in range(S):
                if s_ in scans:
                    assert np.array_equal(got[s_], ref[s_]), (name, s_)
                else:
                    assert (got[s_] == sentinel).all(), (name, s_)

    merged = torch.full((words + 64,), 7.0, dtype=torch.float32, device=DEV)  # 64 words behind the arena
    D.merge_gpu(merged[:words], tile_arena, _dev(first), _dev(tiles), _dev(core), S, T, K, NC, cap, 4)
    host = merged.cpu().numpy()
    assert (host[words:].view(np.uint32) == sentinel).all()
    assert_planes(host, (0, 1))

    # scan 1 alone into its rows of a sentinel arena: scan 0's rows are untouched
    L = importlib.import_module("3dioumatch_amd._lib")
    R = importlib.import_module("3dioumatch_amd.records")
    merged = torch.full((words,), 7.0, dtype=torch.float32, device=DEV)
    keep = [_dev(first[1:]), _dev(tiles[1:]), _dev(core)]
    a = R.ScanMergeArgs()
    a.S, a.K, a.NC, a.cap, a.max_tiles = 1, K, NC, cap, 4
    a.first, a.tiles, a.core = (t.data_ptr() for t in keep)
    lin, _ = D.arena_layout(T, K, NC)
    for plane in D.PLANES:
        setattr(a, plane + "_in", tile_arena.data_ptr() + 4 * lin[plane][0])
    for plane, (at, shape) in layout.items():
        setattr(a, plane, merged.data_ptr() + 4 * (at + int(np.prod(shape[1:]))))  # row 1 of the plane
    L.check(L.lib.scene_detections_merge(ctypes.byref(a), L.current_stream_ptr(DEV)), "scene_detections_merge")
    assert_planes(merged.cpu().numpy(), (1,))

    # refusals, without a launch
    with pytest.raises(ValueError, match="cap"):
        D.merge_gpu(merged, tile_arena, _dev(first), _dev(tiles), _dev(core), S, T, K, NC, 4 * K - 1, 4)
    a = R.ScanMergeArgs()
    for f, _ in a._fields_[5:]:
        setattr(a, f, tile_arena.data_ptr())
    invalid = 1  # hipErrorInvalidValue
    for S_, K_, NC_, cap_, mt_ in ((2, K, NC, 4 * K - 1, 4), (2, D.MAX_K + 1, NC, 8 * D.MAX_K, 4), (2, K, -1, cap, 4),
                                   (0, K, NC, cap, 4)):
        a.S, a.K, a.NC, a.cap, a.max_tiles = S_, K_, NC_, cap_, mt_
        assert L.lib.scene_detections_merge(ctypes.byref(a), None) == invalid
    a.S, a.K, a.NC, a.cap, a.max_tiles = 2, K, NC, cap, 4
    a.core = None
    assert L.lib.scene_detections_merge(ctypes.byref(a), None) == invalid
    assert L.lib.scene_detections_merge(None, None) == invalid
    torch.cuda.synchronize()


# ------------------------------------------------------------------ detect_tiled(), end to end
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
    """tests/test_scan_detect_gpu.py's: the small detector, 6 synthetic scans of 25 000 rows, 20 000
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


@pytest.mark.parametrize("per_class", [True, False])
def test_one_tile_per_scan_is_detect_on_the_parent(run_setup, per_class):
    V, SC, ST, D = _mods()
    engine, store, cfg, thresh = run_setup
    cd = _config_dict(cfg, per_class_proposal=per_class, conf_thresh=thresh)
    tiles = ST.TileStore.from_store(store, (50.0, 50.0), overlap=1.0)  # larger than every scan
    assert tiles.tiles.tolist() == [1] * 6 and np.isinf(tiles.window).all() and np.isinf(tiles.core).all()
    assert torch.equal(tiles.dev["cloud"].view(torch.int32), store.dev["cloud"].view(torch.int32))
    want = V.detect(engine, SC.ScanLoader(store, 20000, seed=2), cd, batch_size=4, counter=5)
    found = V.detect_tiled(engine, SC.ScanLoader(tiles, 20000, seed=2), cd, batch_size=4, counter=5)
    assert isinstance(found, D.TiledDetections) and found.names == store.names and found.cap == found.K
    got, ref = found.planes(), want.planes()
    print("kept per scan:", ref["count"].tolist())
    assert ref["count"].sum() > 0
    for name in ("count", "proposal", "cls", "score", "box", "corners"):
        assert got[name].shape == ref[name].shape
        assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32),
                              np.ascontiguousarray(ref[name]).view(np.uint32)), name
    for s in range(6):
        c = int(got["count"][s])
        assert (got["tile"][s, :c] == s).all() and not got["tile"][s, c:].any()


def test_two_by_two_is_host_merge_of_detect_on_the_tiles(run_setup, tmp_path):
    V, SC, ST, D = _mods()
    engine, store, cfg, thresh = run_setup
    cd = _config_dict(cfg, per_class_proposal=True, conf_thresh=thresh)
    tiles = ST.TileStore.from_store(store, (4.5, 3.5), overlap=1.0)  # the 8 m x 6 m rooms: 2 x 2
    assert tiles.tiles.tolist() == [4] * 6 and len(tiles) == 24
    loader = SC.ScanLoader(tiles, 20000, seed=2)
    per_tile = V.detect(engine, loader, cd, batch_size=8, counter=3)
    found = V.detect_tiled(engine, loader, cd, batch_size=8, counter=3)
    assert torch.equal(found.tiles.arena.view(torch.int32), per_tile.arena.view(torch.int32))
    want = D.host_merge(per_tile.planes(), tiles.first, tiles.tiles, tiles.core)
    got = found.planes()
    assert found.cap == 4 * found.K and got["tile"].shape == (6, found.cap)
    for name in D.MERGED_PLANES:
        assert got[name].shape == want[name].shape, name
        assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32),
                              np.ascontiguousarray(want[name]).view(np.uint32)), name
    kept, packed = int(got["count"].sum()), int(per_tile.planes()["count"].sum())
    print("owned %d of the tiles' %d rows" % (kept, packed))
    assert 0 < kept < packed  # some row is kept and some row is dropped by ownership
    for s in range(6):  # every owned centre lies in its tile's core, tiles in store order
        c = int(got["count"][s])
        t = got["tile"][s, :c]
        assert (np.diff(t) >= 0).all() and t.min() >= tiles.first[s] and t.max() < tiles.first[s] + 4
        for r in range(c):
            assert ST.in_box(got["box"][s, r, 0:2], tiles.core[t[r]])
    found.save(str(tmp_path))
    with np.load(str(tmp_path / "scan0003.npz")) as f:
        assert int(f["count"]) == got["count"][3] and f["window"].shape == (4, 4) and int(f["tile_first"]) == 12
    assert len(found.as_map_cls()[2]) == cfg.num_class * int(got["count"][2])


def test_detect_tiled_is_reproducible_and_does_not_synchronise(run_setup):
    V, SC, ST, D = _mods()
    engine, store, cfg, thresh = run_setup
    cd = _config_dict(cfg, per_class_proposal=False, conf_thresh=thresh)
    tiles = ST.TileStore.from_store(store, (4.5, 3.5), overlap=1.0)
    loader = SC.ScanLoader(tiles, 20000, seed=2)
    first = V.detect_tiled(engine, loader, cd, batch_size=8, counter=1)  # warm-up: graphs captured
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
        second = V.detect_tiled(engine, loader, cd, batch_size=8, counter=1)  # raises nothing
        with pytest.raises(RuntimeError):
            second[0]   # reading is the first synchronising call
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.equal(first.arena.view(torch.int32), second.arena.view(torch.int32))
    assert torch.equal(first.tiles.arena.view(torch.int32), second.tiles.arena.view(torch.int32))
    assert second[0]["count"] == first[0]["count"]


# ------------------------------------------------------------------ poisoned allocations
@pytest.mark.parametrize("fill", dirty_memory.FILLS, ids=dirty_memory.FILL_IDS)
def test_bindings_on_poisoned_allocations(fill):
    _, SC, ST, D = _mods()
    clouds = edge_clouds(6)
    parent = SC.ScanStore(clouds, DEV, "scannet")
    d = parent.dev
    G = 2  # more segments than any scan has: their partials and counts are never read / written as 0
    grid = ST.tile_grid(ST.host_bounds(clouds), TILE, OVERLAP)
    planes, first, tiles, core, _ = hand_made_tiles(3)
    T, K = planes["proposal"].shape
    tile_arena = _arena_of(D, planes, D.arena_layout, T, K, 3)
    dev = [_dev(x) for x in (grid["parent"], grid["window"], first, tiles, core)]

    def run():
        bounds = ST.scan_bounds_gpu(d["cloud"], d["offset"], d["count"], G)
        counts = ST.tile_count_gpu(d["cloud"], d["offset"], d["count"], dev[0], dev[1], G)
        built = ST.select_tiles(grid, counts.cpu().numpy().sum(1), 1)
        count, offset, base = ST.gather_bases(counts.cpu().numpy()[built])
        crops = ST.tile_gather_gpu(d["cloud"], d["offset"], d["count"], dev[0][_dev(built)], dev[1][_dev(built)], _dev(base),
                                   int(count.sum()), G)
        store = ST.TileStore.from_store(parent, TILE, overlap=OVERLAP)
        merged = D.new_merged_arena(2, 4 * K, 3, DEV)
        D.merge_gpu(merged, tile_arena, dev[2], dev[3], dev[4], 2, T, K, 3, 4 * K, 4)
        torch.cuda.synchronize()
        return bounds, counts, crops, store.dev["cloud"], store.dev["floor"], merged

    clean = run()
    with dirty_memory.poisoned(fill) as p:
        dirty = run()
    assert p.count >= 6  # partials, bounds, crops (twice), floors, the merged arena
    for name, c, x in zip(("bounds", "counts", "crops", "store rows", "store floors", "merged"), clean, dirty):
        assert c.shape == x.shape and torch.equal(c.view(torch.int32), x.view(torch.int32)), name
    assert torch.equal(clean[2].view(torch.int32), clean[3].view(torch.int32))
