"""The voxel downsample on the MI355X: the three launchers against host_voxels launch by launch (every
shared case, 3 and 6 columns, both keep modes), VoxelStore.from_store against the host path field by
field with one device-to-host copy, two constructions bit-equal, the launchers on dirty scratch and
on poisoned allocations, the refusals, and the store under ScanLoader, TileStore and detect()."""
import contextlib
import ctypes
import importlib

import numpy as np
import pytest
import torch

import dirty_memory
import scan_voxel_cases as cases
from conftest import load_pkg
from scan_voxel_cases import KEEPS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INVALID = 1  # hipErrorInvalidValue
TAIL = 64    # words behind every pre-filled buffer: nothing may be written there


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.scan_data"),
            importlib.import_module("3dioumatch_amd.votenet.scan_tiles"),
            importlib.import_module("3dioumatch_amd.votenet.scan_voxels"))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_floor(got, want):  # tests/test_scan_tiles_gpu.py's: the sign of a zero floor is unspecified
    got, want = np.float32(got), np.float32(want)
    return got == want and (got.tobytes() == want.tobytes() or got == 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _filled(shape, dtype, byte):
    """(view, whole): a tensor of `shape` with TAIL elements behind it, every byte `byte`"""
    n = int(np.prod(shape))
    whole = torch.empty(n + TAIL, dtype=dtype, device=DEV)
    whole.view(torch.uint8).fill_(byte)
    return whole[:n].view(shape), whole


def _launches(SV, ST, store, voxel, keep, byte=None):
    """mark, count, gather as VoxelStore.from_store chains them; with `byte` every buffer the launches
    write arrives filled with it.  (counts (S, G), outside (S,), rows, source, count, offset)"""
    d, S, C = store.dev, len(store), store.columns
    G = ST._segments(store.count)
    given, wholes = {}, []
    if byte is not None:
        total = sum(SV.voxel_slots(n) for n in store.count)
        for name, shape, dtype in (("scratch", (2 * total,), torch.int64), ("slot", (int(store.count.sum()),), torch.int32),
                                   ("table", (S * G + S,), torch.int32)):
            given[name], whole = _filled(shape, dtype, byte)
            wholes.append((name, whole, int(np.prod(shape))))
    mark = SV.voxel_mark_gpu(d["cloud"], d["offset"], d["count"], store.count, voxel, keep, G, **given)
    counts = SV.voxel_count_gpu(d["cloud"], d["offset"], d["count"], voxel, keep, mark, G)
    assert counts.shape == (S, G) and counts.dtype == torch.int32
    host_counts, outside = counts.cpu().numpy(), mark["outside"].cpu().numpy()
    count, offset, base = ST.gather_bases(host_counts)
    rows = int(count.sum())
    outs = {}
    if byte is not None:
        for name, shape, dtype in (("out", (rows, C), torch.float32), ("source", (rows,), torch.int32)):
            outs[name], whole = _filled(shape, dtype, byte)
            wholes.append((name, whole, int(np.prod(shape))))
    out, source = SV.voxel_gather_gpu(d["cloud"], d["offset"], d["count"], voxel, keep, mark, _dev(base), rows, G, **outs)
    torch.cuda.synchronize()
    for name, whole, n in wholes:
        assert (whole[n:].view(torch.uint8) == byte).all(), "%s: written behind its end" % name
    slot = mark["slot"].cpu().numpy()
    for s, (o, n) in enumerate(zip(store.offset, store.count)):  # every row has a slot inside its scan's run
        assert (slot[o:o + n] >= 0).all() and (slot[o:o + n] < SV.voxel_slots(n)).all(), s
    return host_counts, outside, out, source, count, offset


# ------------------------------------------------------------------ launch by launch
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("columns", [3, 6])
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_launch_by_launch(case, columns, keep):
    _, SC, ST, SV = _mods()
    clouds, voxel, want = cases.clouds(case, columns), cases.voxel(case), cases.kept(case, keep)
    store = SC.ScanStore(clouds, DEV, "scannet")
    counts, outside, out, source, count, offset = _launches(SV, ST, store, voxel, keep)
    print("%s: kept %s of %s rows" % (case, count.tolist(), store.count.tolist()))
    assert not outside.any()
    assert counts.sum(1).tolist() == [len(k) for k in want]
    for s, k in enumerate(want):  # the table segment by segment
        assert counts[s].tolist() == np.bincount(k // ST.SEGMENT, minlength=counts.shape[1]).tolist(), s
    assert out.shape == (int(count.sum()), columns) and out.dtype == torch.float32
    assert np.array_equal(bits(out.cpu().numpy()), bits(np.concatenate([c[k] for c, k in zip(clouds, want)])))
    assert source.dtype == torch.int32 and np.array_equal(source.cpu().numpy(), np.concatenate(want))
    if case == "all_distinct":  # the output is the input
        assert torch.equal(out.view(torch.int32), store.dev["cloud"].view(torch.int32))


# ------------------------------------------------------------------ the store
@contextlib.contextmanager
def host_reads():
    """Counts the calls that copy a device tensor to the host.  (torch's sync debug mode, which the
    detect tests use, also flags the uploads of pageable host tables, of which the construction has
    several: it cannot count the reads alone.)"""
    seen = []
    names = ("cpu", "item", "tolist", "numpy", "__array__")
    real = {n: getattr(torch.Tensor, n) for n in names}
    real_to, real_sync = torch.Tensor.to, torch.cuda.synchronize

    def wrap(name):
        def call(self, *a, **k):
            if self.is_cuda:
                seen.append(name)
            return real[name](self, *a, **k)
        return call

    def to(self, *a, **k):
        out = real_to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            seen.append("to")
        return out

    def sync(*a, **k):
        seen.append("synchronize")
        return real_sync(*a, **k)

    for n in names:
        setattr(torch.Tensor, n, wrap(n))
    torch.Tensor.to, torch.cuda.synchronize = to, sync
    try:
        yield seen
    finally:
        for n in names:
            setattr(torch.Tensor, n, real[n])
        torch.Tensor.to, torch.cuda.synchronize = real_to, real_sync


def _assert_store_is_the_host_path(SC, SV, store, clouds, voxel, keep):
    want = SV.host_voxels(clouds, voxel, keep)
    rows = [c[k] for c, k in zip(clouds, want)]
    assert store.count.dtype == np.int32 and store.count.tolist() == [len(k) for k in want]
    assert store.offset.dtype == np.int64
    assert store.offset.tolist() == np.concatenate([[0], np.cumsum(store.count, dtype=np.int64)[:-1]]).tolist()
    assert sorted(store.dev) == ["cloud", "count", "floor", "offset", "source"]
    flat = store.dev["cloud"].cpu().numpy()
    assert flat.shape == (int(store.count.sum()), clouds[0].shape[1])
    assert np.array_equal(bits(flat), bits(np.concatenate(rows)))
    assert np.array_equal(store.dev["count"].cpu().numpy(), store.count)
    assert np.array_equal(store.dev["offset"].cpu().numpy(), store.offset)
    assert store.dev["source"].dtype == torch.int32
    assert np.array_equal(store.dev["source"].cpu().numpy(), np.concatenate(want))
    assert store.source.dtype == np.int32 and np.array_equal(store.source, np.concatenate(want))
    floor = store.dev["floor"].cpu().numpy()
    for s, r in enumerate(rows):
        assert same_floor(floor[s], SC.host_floor(r[:, 2])), s
        assert np.array_equal(bits(store.clouds[s]), bits(r))  # the lazy host rows
    assert np.array_equal(bits(store.floor), bits(floor))
    return rows


@pytest.mark.parametrize("keep", KEEPS)
def test_store_is_the_host_path_with_one_host_read(keep):
    _, SC, ST, SV = _mods()
    clouds = cases.clouds("boundary", 6)
    names = ["scan_%d" % n for n in cases.BOUNDARY_SIZES]
    parent = SC.ScanStore(clouds, DEV, "scannet", names=names)
    host = SV.VoxelStore.from_store(SC.ScanStore(clouds, None, "scannet", names=names), cases.BOUNDARY_VOXEL, keep)
    torch.cuda.synchronize()
    with host_reads() as seen:
        store = SV.VoxelStore.from_store(parent, cases.BOUNDARY_VOXEL, keep=keep)
    assert seen == ["cpu"], seen  # the counts and the out-of-range counters, in one copy
    assert isinstance(store, SC.ScanStore) and store.device == DEV and store.names == names
    assert store.source_store is parent and store.voxel == (cases.BOUNDARY_VOXEL,) * 3 and store.keep == keep
    assert store.columns == 6 and store.dataset == "scannet" and len(store) == len(clouds)
    assert store._clouds is None and store._floor is None and store._source is None  # filled at first use
    _assert_store_is_the_host_path(SC, SV, store, clouds, cases.BOUNDARY_VOXEL, keep)
    assert np.array_equal(store.count, host.count) and np.array_equal(store.offset, host.offset)
    assert np.array_equal(store.source, host.source)
    assert all(same_floor(a, b) for a, b in zip(store.floor, host.floor))


@pytest.mark.parametrize("keep", KEEPS)
def test_two_constructions_are_bit_equal(keep):
    _, SC, ST, SV = _mods()
    clouds = cases.clouds("boundary", 3)[:9] + cases.clouds("edge", 3) + cases.clouds("one_cell", 3)
    parent = SC.ScanStore(clouds, DEV, "scannet")
    a = SV.VoxelStore.from_store(parent, cases.EDGE_VOXEL, keep=keep)
    b = SV.VoxelStore.from_store(parent, cases.EDGE_VOXEL, keep=keep)
    assert np.array_equal(a.count, b.count)
    for k in ("cloud", "source", "floor", "count", "offset"):
        assert a.dev[k].data_ptr() != b.dev[k].data_ptr()
        assert torch.equal(a.dev[k].view(torch.int32), b.dev[k].view(torch.int32)), k
    _assert_store_is_the_host_path(SC, SV, a, clouds, cases.EDGE_VOXEL, keep)


# ------------------------------------------------------------------ dirty scratch, poisoned allocations
@pytest.mark.parametrize("keep", KEEPS)
def test_launchers_on_dirty_scratch(keep):
    _, SC, ST, SV = _mods()
    clouds = cases.clouds("boundary", 6)[:9] + cases.clouds("edge", 6)
    store = SC.ScanStore(clouds, DEV, "scannet")
    clean = _launches(SV, ST, store, cases.EDGE_VOXEL, keep)
    assert np.array_equal(clean[3].cpu().numpy(), np.concatenate(SV.host_voxels(clouds, cases.EDGE_VOXEL, keep)))
    for byte in (0x5A, 0xFF):
        dirty = _launches(SV, ST, store, cases.EDGE_VOXEL, keep, byte=byte)
        assert np.array_equal(clean[0], dirty[0]) and np.array_equal(clean[1], dirty[1]), byte
        assert torch.equal(clean[2].view(torch.int32), dirty[2].view(torch.int32)), byte
        assert torch.equal(clean[3], dirty[3]), byte


@pytest.mark.parametrize("fill", dirty_memory.FILLS, ids=dirty_memory.FILL_IDS)
def test_store_on_poisoned_allocations(fill):
    _, SC, ST, SV = _mods()
    clouds = cases.clouds("boundary", 6)[:9] + cases.clouds("edge", 6)
    parent = SC.ScanStore(clouds, DEV, "scannet")

    def run(keep):
        store = SV.VoxelStore.from_store(parent, cases.EDGE_VOXEL, keep=keep)
        torch.cuda.synchronize()
        return store.dev["cloud"], store.dev["source"], store.dev["floor"], store.dev["count"]

    for keep in KEEPS:
        clean = run(keep)
        with dirty_memory.poisoned(fill) as p:
            dirty = run(keep)
        assert p.count >= 2  # the rows and the floors
        for name, c, x in zip(("rows", "source", "floors", "count"), clean, dirty):
            assert c.shape == x.shape and torch.equal(c.view(torch.int32), x.view(torch.int32)), (keep, name)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("keep", KEEPS)
def test_a_scan_out_of_range_is_refused_and_the_others_are_unaffected(keep):
    _, SC, ST, SV = _mods()
    g = np.random.default_rng(41)
    near = [(g.random((n, 3)) * 40 - 20).astype(np.float32) for n in (500, 70000)]
    far = (g.random((3000, 3)) * 40 - 20).astype(np.float32)
    far[[5, 1500, 2999], [0, 1, 2]] = [3e6, -3e6, 3e6]
    parent = SC.ScanStore([near[0], far, near[1]], DEV, "scannet", names=["near", "far", "nearer"])
    with pytest.raises(ValueError, match=r"beyond 2\^20 cells.*: far \(3\)$"):
        SV.VoxelStore.from_store(parent, 1.0, keep=keep)
    # launch by launch: the scan's rows out of range are counted and dropped, the other scans' results stand
    counts, outside, out, source, count, offset = _launches_with_outside(SV, ST, parent, 1.0, keep)
    assert outside.tolist() == [0, 3, 0]
    want = SV.host_voxels(near, 1.0, keep)
    for s, k in ((0, want[0]), (2, want[1])):
        assert count[s] == len(k)
        assert np.array_equal(source[offset[s]:offset[s] + count[s]].cpu().numpy(), k)
    inside = np.delete(far, [5, 1500, 2999], 0)
    assert count[1] == len(SV.host_voxels([inside], 1.0, keep)[0])
    # and left out, the store is built
    rest = SC.ScanStore(near, DEV, "scannet", names=["near", "nearer"])
    _assert_store_is_the_host_path(SC, SV, SV.VoxelStore.from_store(rest, 1.0, keep=keep), near, 1.0, keep)


def _launches_with_outside(SV, ST, store, voxel, keep):
    """_launches for a store with rows out of range: those rows have slot -1"""
    d, G = store.dev, ST._segments(store.count)
    mark = SV.voxel_mark_gpu(d["cloud"], d["offset"], d["count"], store.count, voxel, keep, G)
    counts = SV.voxel_count_gpu(d["cloud"], d["offset"], d["count"], voxel, keep, mark, G).cpu().numpy()
    count, offset, base = ST.gather_bases(counts)
    out, source = SV.voxel_gather_gpu(d["cloud"], d["offset"], d["count"], voxel, keep, mark, _dev(base),
                                      int(count.sum()), G)
    assert int((mark["slot"] < 0).sum()) == int(mark["outside"].sum())
    return counts, mark["outside"].cpu().numpy(), out, source, count, offset


def test_entry_points_refuse_without_a_launch():
    _, SC, ST, SV = _mods()
    L = importlib.import_module("3dioumatch_amd._lib")
    R = importlib.import_module("3dioumatch_amd.records")
    store = SC.ScanStore(cases.clouds("edge", 3), DEV, "scannet")
    d, G = store.dev, 1
    mark = SV.voxel_mark_gpu(d["cloud"], d["offset"], d["count"], store.count, 0.25, "first", G)
    counts = SV.voxel_count_gpu(d["cloud"], d["offset"], d["count"], 0.25, "first", mark, G)
    torch.cuda.synchronize()
    before = [t.clone() for t in (mark["scratch"], mark["slot"], mark["table"])]
    P = int(store.count.sum())  # full-sized outputs: in bounds even if an entry point did launch
    base = torch.zeros((1, G), dtype=torch.int64, device=DEV)
    out, source = torch.zeros((P, 3), device=DEV), torch.zeros(P, dtype=torch.int32, device=DEV)

    def record():
        return SV._mark_record(d["cloud"], d["offset"], d["count"], (0.25, 0.25, 0.25), "first", mark, G)

    def refused(change):
        a = record()
        change(a)
        c, g = R.ScanVoxelCountArgs(), R.ScanVoxelGatherArgs()
        c.mark, c.counts = a, counts.data_ptr()
        g.mark, g.rows = a, P
        g.base, g.out, g.source = base.data_ptr(), out.data_ptr(), source.data_ptr()
        return [L.lib.scene_scan_voxel_mark(ctypes.byref(a), None), L.lib.scene_scan_voxel_count(ctypes.byref(c), None),
                L.lib.scene_scan_voxel_gather(ctypes.byref(g), None)]

    def setter(**fields):
        def change(a):
            for k, v in fields.items():
                setattr(a, k, v)
        return change

    def voxel(x, v):
        def change(a):
            a.voxel[x] = v
        return change

    changes = [setter(S=0), setter(S=-1), setter(S=65536), setter(C=4), setter(C=0), setter(max_segments=0),
               setter(total_slots=0), setter(scratch_bytes=16 * mark["total_slots"] - 1), setter(scratch_bytes=0),
               setter(scratch=mark["scratch"].data_ptr() + 4), voxel(0, 0.0), voxel(1, -1.0), voxel(2, float("nan")),
               voxel(0, float("inf"))]
    changes += [setter(**{name: None}) for name in ("cloud", "offset", "count", "slot_offset", "scratch", "slot", "outside")]
    for change in changes:
        assert refused(change) == [INVALID] * 3
    a = record()
    c, g = R.ScanVoxelCountArgs(), R.ScanVoxelGatherArgs()
    c.mark, g.mark, g.rows = a, a, P
    assert L.lib.scene_scan_voxel_count(ctypes.byref(c), None) == INVALID  # counts NULL
    for name in ("base", "out", "source"):
        g.base, g.out, g.source = base.data_ptr(), out.data_ptr(), source.data_ptr()
        setattr(g, name, None)
        assert L.lib.scene_scan_voxel_gather(ctypes.byref(g), None) == INVALID
    g.base, g.out, g.source = base.data_ptr(), out.data_ptr(), source.data_ptr()
    g.rows = 0
    assert L.lib.scene_scan_voxel_gather(ctypes.byref(g), None) == INVALID
    for entry in ("scene_scan_voxel_mark", "scene_scan_voxel_count", "scene_scan_voxel_gather"):
        assert getattr(L.lib, entry)(None, None) == INVALID
    torch.cuda.synchronize()
    for was, now in zip(before, (mark["scratch"], mark["slot"], mark["table"])):
        assert torch.equal(was, now)  # nothing ran
    assert not out.any() and not source.any()
    with pytest.raises(ValueError, match="voxel"):
        SV.VoxelStore.from_store(store, (0.1, 0.0, 0.1))
    with pytest.raises(ValueError, match="keep"):
        SV.VoxelStore.from_store(store, 0.1, keep="centroid")
    with pytest.raises(ValueError, match="TileStore"):
        SV.VoxelStore.from_store(ST.TileStore.from_store(store, 5000.0), 0.1)  # (the scan spans 2 km)


# ------------------------------------------------------------------ downstream
@pytest.mark.parametrize("use_color", [False, True])
def test_batches_of_a_voxel_store_are_those_of_a_store_of_the_kept_rows(use_color):
    _, SC, ST, SV = _mods()
    clouds = cases.clouds("boundary", 6)[4:8] + cases.clouds("edge", 6)
    store = SV.VoxelStore.from_store(SC.ScanStore(clouds, DEV, "scannet"), cases.BOUNDARY_VOXEL, keep="nearest")
    kept = SV.host_voxels(clouds, cases.BOUNDARY_VOXEL, "nearest")
    plain = SC.ScanStore([c[k] for c, k in zip(clouds, kept)], DEV, "scannet", names=store.names)
    N = 512  # above and below the scans' counts
    a = SC.ScanLoader(store, N, use_color=use_color, seed=5)
    b = SC.ScanLoader(plain, N, use_color=use_color, seed=5)
    for ids, counter in ((np.arange(5), 0), ([4, 0, 3], 11)):
        got, want = a.batch(ids, counter), b.batch(ids, counter)
        assert torch.equal(got["point_clouds"].view(torch.int32), want["point_clouds"].view(torch.int32))
        assert torch.equal(got["scan_idx"], want["scan_idx"])


def test_a_tile_store_of_a_voxel_store_is_host_tiles_of_the_kept_rows():
    _, SC, ST, SV = _mods()
    clouds = cases.clouds("anisotropic", 6) + cases.clouds("boundary", 6)[7:9]
    store = SV.VoxelStore.from_store(SC.ScanStore(clouds, DEV, "scannet", names=["room", "x", "y"]), cases.ANISO_VOXEL)
    tile, overlap = (2.5, 2.5), 0.5
    tiles = ST.TileStore.from_store(store, tile, overlap=overlap)
    kept = [c[k] for c, k in zip(clouds, SV.host_voxels(clouds, cases.ANISO_VOXEL))]
    grid = ST.tile_grid(ST.host_bounds(kept), tile, overlap)
    built, crops = ST.host_tiles(kept, grid)
    assert tiles.source is store and tiles.parent_names == ["room", "x", "y"] and tiles.tiles[0] == 4
    assert np.array_equal(tiles.parent, grid["parent"][built])
    assert tiles.count.tolist() == [len(c) for c in crops]
    assert np.array_equal(bits(tiles.dev["cloud"].cpu().numpy()), bits(np.concatenate(crops)))
    floor = tiles.dev["floor"].cpu().numpy()
    assert all(same_floor(floor[t], SC.host_floor(c[:, 2])) for t, c in enumerate(crops))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(tiles.clouds, crops))  # through the lazy host rows


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


def test_detect_on_a_voxel_store_is_detect_on_the_kept_rows():
    """tests/test_scan_detect_gpu.py's small detector on two scans that each hold a room and a second,
    overlapping copy of a part of it"""
    V, SC, ST, SV = _mods()
    I = importlib.import_module("3dioumatch_amd.votenet.inference")
    step = importlib.import_module("3dioumatch_amd.votenet.step")
    cfg = V.scannet_config()
    det = step.build_detector(cfg, seed=0).to(DEV)
    _randomize_bn(det, 11)
    engine = I.InferenceEngine(det.eval())
    rooms = SC.synthetic_clouds(2, 25000, seed=3, color=False)
    clouds = [np.concatenate([r, r[3000:15000]]) for r in rooms]  # the copy's rows fall into occupied cells
    voxel = 0.05
    store = SV.VoxelStore.from_store(SC.ScanStore(clouds, DEV, "scannet"), voxel)
    kept = SV.host_voxels(clouds, voxel)
    assert store.count.tolist() == [len(k) for k in kept] and (store.count <= 25000).all()
    plain = SC.ScanStore([c[k] for c, k in zip(clouds, kept)], DEV, "scannet", names=store.names)
    ep = engine(SC.ScanLoader(plain, 20000, seed=2).batch([0, 1], 0)["point_clouds"])
    thresh = float(torch.softmax(ep["objectness_scores"], -1)[:, :, 1].median())
    cd = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
          "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False, "per_class_proposal": True,
          "conf_thresh": thresh}
    got = V.detect(engine, SC.ScanLoader(store, 20000, seed=2), cd, batch_size=2, counter=5).planes()
    want = V.detect(engine, SC.ScanLoader(plain, 20000, seed=2), cd, batch_size=2, counter=5).planes()
    print("kept per scan:", want["count"].tolist())
    assert want["count"].sum() > 0
    for name in ("count", "proposal", "cls", "score", "box", "corners"):
        assert got[name].shape == want[name].shape
        assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32),
                              np.ascontiguousarray(want[name]).view(np.uint32)), name
