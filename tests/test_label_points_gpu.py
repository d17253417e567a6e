"""label_points on the MI355X, launch by launch: scene_detections_frames against numpy (centre, half
sizes, rank words, cls and the zeroed points bit for bit, cos and sin within one float32 ulp),
scene_points_label against host_label_points fed the device's frames (every shared case, 3 and 6
columns, both prefer modes, cull on and off), the geometric cases against float64, two runs bit-equal,
dirty outputs with a guard tail, poisoned allocations, no host read inside label_points and one at the
first labels[i], the refusals, and detect / detect_tiled end to end with a random-weight detector."""
import contextlib
import ctypes
import importlib

import numpy as np
import pytest
import torch

import dirty_memory
import label_points_cases as cases
from conftest import load_pkg
from label_points_cases import PREFERS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INVALID = 1  # hipErrorInvalidValue
TAIL = 64    # words behind every pre-filled buffer: nothing may be written there


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.scan_data"),
            importlib.import_module("3dioumatch_amd.votenet.detect"),
            importlib.import_module("3dioumatch_amd.votenet.point_labels"))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared cases are read-only


def _filled(shape, dtype, byte):
    """(view, whole, n): a tensor of `shape` with TAIL elements behind it, every byte `byte`"""
    n = int(np.prod(shape))
    whole = torch.empty(n + TAIL, dtype=dtype, device=DEV)
    whole.view(torch.uint8).fill_(byte)
    return whole[:n].view(shape), whole, n


def _planes_dev(case, garbage=None):
    p = cases.planes(case, garbage)
    return {k: _dev(p[k]) for k in ("count", "cls", "score", "box")}


def _launches(PL, case, columns, prefer, min_score=0.0, cull=True, byte=None, garbage=None):
    """frames, then label, as label_points chains them; with `byte` every output and the scratch arrive
    filled with it.  -> {frames, rank, cls, radius, points0 (after the frames launch), instance,
    semantic, points} as numpy arrays"""
    SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
    c = cases.get(case)
    store = SC.ScanStore(cases.clouds(case, columns), DEV, "scannet", names=c["names"])
    d, S, cap = store.dev, len(store), c["cap"]
    P = int(store.count.sum())
    pl = _planes_dev(case, garbage)
    given, wholes = {}, []
    if byte is not None:
        for name, shape, dtype in (("frames", (S, cap, 8), torch.float32), ("points", (S, cap), torch.int32),
                                   ("scratch", (2 * S * cap,), torch.int64), ("instance", (P,), torch.int32),
                                   ("semantic", (P,), torch.int32)):
            given[name], whole, n = _filled(shape, dtype, byte)
            wholes.append((name, whole, n))
    frames, points, scratch = PL.frames_gpu(pl["count"], pl["cls"], pl["score"], pl["box"], c["K"], prefer, min_score,
                                            **{k: given[k] for k in ("frames", "points", "scratch") if k in given})
    rank, cls, radius = PL.scratch_views(scratch, S, cap)
    out = {"frames": frames.cpu().numpy(), "rank": rank.cpu().numpy().view(np.uint64), "cls": cls.cpu().numpy(),
           "radius": radius.cpu().numpy(), "points0": points.cpu().numpy()}
    instance, semantic = PL.label_gpu(d["cloud"], d["offset"], d["count"], PL.max_blocks_of(store.count), pl["count"],
                                      frames, scratch, c["K"], points, cull=cull,
                                      **{k: given[k] for k in ("instance", "semantic") if k in given})
    torch.cuda.synchronize()
    for name, whole, n in wholes:
        assert (whole[n:].view(torch.uint8) == byte).all(), "%s: written behind its end" % name
    out.update(instance=instance.cpu().numpy(), semantic=semantic.cpu().numpy(), points=points.cpu().numpy())
    return out


def _ulps(a, b):
    """float32 steps between two arrays of finite values (sign-magnitude bits to a line)"""
    def line(x):
        u = bits(x).astype(np.int64)
        return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)
    return np.abs(line(a) - line(b))


def _assert_frames(PL, case, got, prefer, min_score):
    """the frames launch against numpy; returns the number of cos / sin values that differ"""
    want = PL.host_frames(cases.planes(case), prefer, min_score)
    assert np.array_equal(bits(got["frames"][..., 2:8]), bits(want["frames"][..., 2:8]))  # centre, half sizes
    cs, ref = got["frames"][..., 0:2], want["frames"][..., 0:2]
    assert np.array_equal(np.isnan(cs), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert (_ulps(cs[ok], ref[ok]) <= 1).all()
    assert not got["points0"].any()
    assert np.array_equal(got["cls"], want["cls"])
    # the rank does not depend on cos and sin beyond their being finite
    assert got["rank"].dtype == np.uint64 and np.array_equal(got["rank"], want["rank"])
    eligible = want["rank"] != 0
    assert (got["radius"][eligible].astype(np.float64) > want["reach"][eligible]).all()  # rounded up and inflated
    assert (got["radius"][eligible].astype(np.float64) <= want["reach"][eligible] * (1 + 2.0 ** -9) + 2.0 ** -100).all()
    assert not got["radius"][~eligible].any()
    return int((bits(cs[ok]) != bits(ref[ok])).sum())


# ------------------------------------------------------------------ launch by launch
@pytest.mark.parametrize("columns", [3, 6])
@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_launch_by_launch(case, columns):
    _, SC, D, PL = _mods()
    c = cases.get(case)
    differing = 0
    for prefer in PREFERS:
        for min_score in cases.min_scores(case):
            ref = cases.want(case, prefer, min_score)
            for cull in (True, False):
                got = _launches(PL, case, columns, prefer, min_score, cull)
                differing += _assert_frames(PL, case, got, prefer, min_score)
                # the restatement on the device's frames
                want = PL.host_label_points(cases.planes(case), c["clouds"], prefer, min_score, frames=got["frames"])
                for k in ("instance", "semantic", "points"):
                    assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (prefer, min_score, cull, k)
                if np.array_equal(bits(np.nan_to_num(got["frames"])), bits(np.nan_to_num(ref["frames"]))):
                    assert np.array_equal(got["instance"], ref["instance"])  # and so the shared result
    print("%s: %d cos / sin values differ from numpy's" % (case, differing))


@pytest.mark.parametrize("seed", cases.GEOMETRIC_SEEDS)
def test_geometric_cases_equal_float64(seed):
    """independent of the frames: every point is at least 1e-4 m from every face plane"""
    _, SC, D, PL = _mods()
    case = "geometric%d" % seed
    for prefer in PREFERS:
        for cull in (True, False):
            got = _launches(PL, case, 3, prefer, cull=cull)
            assert np.array_equal(got["instance"], cases.float64_labels(case, prefer)), (prefer, cull)


@pytest.mark.parametrize("garbage", cases.GARBAGE)
def test_rows_past_count_are_never_read(garbage):
    _, SC, D, PL = _mods()
    for case in ("sizes", "chunks"):
        for prefer in PREFERS:
            clean = _launches(PL, case, 3, prefer)
            dirty = _launches(PL, case, 3, prefer, garbage=garbage)
            for k in clean:
                assert np.array_equal(bits(clean[k]) if clean[k].dtype == np.float32 else clean[k],
                                      bits(dirty[k]) if dirty[k].dtype == np.float32 else dirty[k]), (case, prefer, k)


def test_two_runs_are_bit_equal_and_dirty_outputs_do_not_matter():
    _, SC, D, PL = _mods()
    for case in ("chunks", "cull", "ownership"):
        for prefer in PREFERS:
            first = _launches(PL, case, 6, prefer)
            again = _launches(PL, case, 6, prefer)
            runs = [again] + [_launches(PL, case, 6, prefer, byte=byte) for byte in (0x00, 0x7F, 0xFF)]
            for other in runs:
                for k in ("frames", "rank", "cls", "radius", "points0", "instance", "semantic", "points"):
                    a, b = first[k], other[k]
                    assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                          b.view(np.uint32) if b.dtype == np.float32 else b), (case, prefer, k)


# ------------------------------------------------------------------ label_points
@contextlib.contextmanager
def host_reads():
    """tests/test_scan_voxels_gpu.py's: counts the calls that copy a device tensor to the host"""
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


@pytest.mark.parametrize("case", ["sizes", "chunks"])
def test_label_points_both_layouts_without_a_host_read(case, tmp_path):
    _, SC, D, PL = _mods()
    c = cases.get(case)
    store = SC.ScanStore(cases.clouds(case, 6), DEV, "scannet", names=c["names"])
    found = cases.found(case, _dev(cases.arena(case)))
    torch.cuda.synchronize()
    for prefer in PREFERS:
        with host_reads() as seen:
            labels = PL.label_points(found, store, prefer=prefer)
        assert seen == [], seen
        for t, shape in ((labels.instance, (int(store.count.sum()),)), (labels.semantic, (int(store.count.sum()),)),
                         (labels.points, (len(store), c["cap"]))):
            assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == shape
        assert labels.frames.is_cuda and tuple(labels.frames.shape) == (len(store), c["cap"], 8)
        with host_reads() as seen:
            one = labels[len(store) - 1]
        assert seen == ["cpu"], seen  # the one copy
        with host_reads() as seen:
            labels[0], labels.by_name(c["names"][1]), labels.points_of(1, 0)
            labels.save(str(tmp_path / prefer))
        assert seen == [], seen
        want = PL.host_label_points(cases.planes(case), c["clouds"], prefer, frames=labels.frames.cpu().numpy())
        assert np.array_equal(labels.instance.cpu().numpy(), want["instance"])
        assert np.array_equal(labels.semantic.cpu().numpy(), want["semantic"])
        assert np.array_equal(labels.points.cpu().numpy(), want["points"])
        n = len(c["clouds"][-1])
        assert np.array_equal(one["instance"], want["instance"][-n:]) and np.array_equal(one["points"], want["points"][-1])
        for i, name in enumerate(c["names"]):
            z = np.load(str(tmp_path / prefer / (name + "_labels.npz")))
            assert np.array_equal(z["instance"], labels[i]["instance"]) and str(z["prefer"]) == prefer
            assert np.array_equal(z["points"], want["points"][i, :int(c["planes"]["count"][i])])
        # an arena that is not on the store's device goes through numpy, to the same labels
        host = PL.label_points(cases.found(case, cases.arena(case)), store, prefer=prefer)
        assert isinstance(host.instance, np.ndarray)
        assert np.array_equal(host.instance, cases.want(case, prefer)["instance"])


@pytest.mark.parametrize("fill", dirty_memory.FILLS, ids=dirty_memory.FILL_IDS)
def test_label_points_on_poisoned_allocations(fill):
    _, SC, D, PL = _mods()
    c = cases.get("chunks")
    store = SC.ScanStore(cases.clouds("chunks", 3), DEV, "scannet", names=c["names"])
    found = cases.found("chunks", _dev(cases.arena("chunks")))

    def run(prefer):
        labels = PL.label_points(found, store, prefer=prefer)
        torch.cuda.synchronize()
        return labels._words, labels.frames

    for prefer in PREFERS:
        clean = run(prefer)
        with dirty_memory.poisoned(fill) as p:
            dirty = run(prefer)
        assert p.count >= 1  # the frames
        for a, b in zip(clean, dirty):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), prefer


# ------------------------------------------------------------------ refusals
def test_entry_points_refuse_without_a_launch():
    _, SC, D, PL = _mods()
    L = importlib.import_module("3dioumatch_amd._lib")
    case = "sizes"
    c = cases.get(case)
    store = SC.ScanStore(cases.clouds(case, 3), DEV, "scannet")
    d, S, cap, P = store.dev, len(store), c["cap"], int(store.count.sum())
    pl = _planes_dev(case)
    frames, points, scratch = PL.frames_gpu(pl["count"], pl["cls"], pl["score"], pl["box"], c["K"])
    instance, semantic = PL.label_gpu(d["cloud"], d["offset"], d["count"], PL.max_blocks_of(store.count), pl["count"],
                                      frames, scratch, c["K"], points)
    torch.cuda.synchronize()
    outs = (frames, points, scratch, instance, semantic)
    before = [t.clone() for t in outs]
    need = PL.label_scratch_bytes(S, cap)
    assert need == 16 * S * cap == scratch.numel() * 8

    def frames_record():
        return PL.frames_record(pl["count"], pl["cls"], pl["score"], pl["box"], c["K"], "score", 0.0, frames, points,
                                scratch)

    def label_record():
        return PL.label_record(d["cloud"], d["offset"], d["count"], PL.max_blocks_of(store.count), pl["count"], frames,
                               scratch, c["K"], True, instance, semantic, points)

    def refused(make, entry, **fields):
        a = make()
        for k, v in fields.items():
            setattr(a, k, v)
        return getattr(L.lib, entry)(ctypes.byref(a), None)

    shared = [dict(S=0), dict(S=-1), dict(S=65536), dict(K=0), dict(K=D.MAX_K + 1), dict(cap=0), dict(cap=-3),
              dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(scratch=scratch.data_ptr() + 4), dict(scratch=None)]
    only_frames = [dict(prefer=2), dict(prefer=-1), dict(min_score=float("nan")), dict(min_score=float("inf")),
                   dict(min_score=-float("inf")), dict(NC=-1)]
    only_frames += [{name: None} for name in ("count", "cls", "score", "box", "frames", "points")]
    only_label = [dict(C=4), dict(C=0), dict(C=7), dict(max_blocks=0)]
    only_label += [{name: None} for name in ("cloud", "offset", "count", "rows", "frames", "instance", "semantic", "points")]
    for fields in shared + only_frames:
        assert refused(frames_record, "scene_detections_frames", **fields) == INVALID, fields
    for fields in shared + only_label:
        assert refused(label_record, "scene_points_label", **fields) == INVALID, fields
    for entry in ("scene_detections_frames", "scene_points_label"):
        assert getattr(L.lib, entry)(None, None) == INVALID
    torch.cuda.synchronize()
    for was, now in zip(before, outs):
        assert torch.equal(was.view(torch.int32), now.view(torch.int32))  # nothing ran
    found = cases.found(case, _dev(cases.arena(case)))
    with pytest.raises(ValueError, match="prefer"):
        PL.label_points(found, store, prefer="best")
    with pytest.raises(ValueError, match="min_score"):
        PL.label_points(found, store, min_score=float("nan"))
    with pytest.raises(ValueError, match="scan 0 is 'sizes_0' in the detections and 'scan0000' in the store"):
        PL.label_points(found, store)


# ------------------------------------------------------------------ end to end
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


@pytest.fixture(scope="module")
def run_setup():
    """tests/test_scan_detect_gpu.py's small detector on two synthetic scans of 25 000 rows, a
    confidence threshold at the median objectness"""
    V, SC, D, PL = _mods()
    I = importlib.import_module("3dioumatch_amd.votenet.inference")
    step = importlib.import_module("3dioumatch_amd.votenet.step")
    cfg = V.scannet_config()
    det = step.build_detector(cfg, seed=0).to(DEV)
    _randomize_bn(det, 11)
    raw = SC.ScanStore(SC.synthetic_clouds(2, 25000, seed=3, color=False), DEV, "scannet", names=["room_a", "room_b"])
    engine = I.InferenceEngine(det.eval())
    ep = engine(SC.ScanLoader(raw, 20000, seed=2).batch([0, 1], 0)["point_clouds"])
    thresh = float(torch.softmax(ep["objectness_scores"], -1)[:, :, 1].median())
    return engine, raw, cfg, thresh


def _config_dict(cfg, **over):
    cd = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
          "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False, "per_class_proposal": True,
          "conf_thresh": 0.05}
    cd.update(over)
    return cd


def _assert_end_to_end(PL, found, raw, prefer, tmp_path):
    labels = PL.label_points(found, raw, prefer=prefer)
    planes = found.planes()
    want = PL.host_label_points({k: planes[k] for k in ("count", "cls", "score", "box")}, raw.clouds, prefer,
                                frames=labels.frames.cpu().numpy())
    instance, points = labels.instance.cpu().numpy(), labels.points.cpu().numpy()
    assert np.array_equal(instance, want["instance"])
    assert np.array_equal(labels.semantic.cpu().numpy(), want["semantic"])
    assert np.array_equal(points, want["points"])
    assert (instance >= 0).sum() > 0
    for s, (o, n) in enumerate(zip(raw.offset, raw.count)):
        assert points[s].sum() + (instance[o:o + n] == -1).sum() == n
        assert not points[s, int(planes["count"][s]):].any()
    labels.save(str(tmp_path / prefer))
    for i, name in enumerate(raw.names):
        z = np.load(str(tmp_path / prefer / (name + "_labels.npz")))
        assert np.array_equal(z["instance"], labels[i]["instance"])
        assert np.array_equal(z["semantic"], labels[i]["semantic"])
        assert np.array_equal(z["points"], points[i, :int(planes["count"][i])])
        assert str(z["prefer"]) == prefer and float(z["min_score"]) == 0.0
    return labels


@pytest.mark.parametrize("per_class", [True, False])
def test_detect_on_a_voxel_store_labels_the_raw_store(run_setup, per_class, tmp_path):
    V, SC, D, PL = _mods()
    engine, raw, cfg, thresh = run_setup
    thin = V.VoxelStore.from_store(raw, 0.1)
    assert (thin.count < raw.count).all()
    cd = _config_dict(cfg, per_class_proposal=per_class, conf_thresh=thresh)
    found = V.detect(engine, SC.ScanLoader(thin, 20000, seed=2), cd, batch_size=2, counter=5)
    for prefer in PREFERS:
        labels = _assert_end_to_end(PL, found, raw, prefer, tmp_path)
    print("boxes per scan:", found.planes()["count"].tolist(), "labelled:", int((labels.instance >= 0).sum()))


def test_detect_tiled_labels_the_parent_store(run_setup, tmp_path):
    V, SC, D, PL = _mods()
    ST = importlib.import_module("3dioumatch_amd.votenet.scan_tiles")
    engine, raw, cfg, thresh = run_setup
    tiles = ST.TileStore.from_store(raw, (4.5, 3.5), overlap=1.0)  # the 8 m x 6 m rooms: 2 x 2
    cd = _config_dict(cfg, conf_thresh=thresh)
    tiled = V.detect_tiled(engine, SC.ScanLoader(tiles, 20000, seed=2), cd, batch_size=8, counter=3, seam_nms=True)
    assert tiled.store.source is raw and tiled.cap == 4 * tiled.K
    for prefer in PREFERS:
        _assert_end_to_end(PL, tiled, tiled.store.source, prefer, tmp_path)
