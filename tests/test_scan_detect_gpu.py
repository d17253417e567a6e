"""The label-free scan path on the MI355X: scene_scan_prepare against host_floor, scene_scan_batch_build
against ScanLoader.host_batch and against the labeled loader's eval batches, scene_detections_pack
against parse_predictions on the same end points, detect() end to end -- equal to engine.run +
parse_predictions, reproducible, and without a synchronising call in its loop -- and the three bindings
on poisoned allocations."""
import importlib

import numpy as np
import pytest
import torch

import dirty_memory
from conftest import load_pkg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N = 2048


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.scan_data"),
            importlib.import_module("3dioumatch_amd.votenet.detect"))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_floor(got, want):
    got, want = np.float32(got), np.float32(want)
    return got == want and (got.tobytes() == want.tobytes() or got == 0)


# ------------------------------------------------------------------ scene_scan_prepare
PREPARE_SIZES = (1, 2, 63, 64, 65, 101, 102, 1025, 4099, 70001)


def _prepare_clouds(columns):
    """one cloud per size of PREPARE_SIZES; what z holds depends on the scan (see the comments)"""
    g = np.random.default_rng(77)
    clouds = []
    for n in PREPARE_SIZES:
        c = (g.random((n, columns)) * 4 - 1).astype(np.float32)  # mixed sign
        if n == 102:     # +-0.0 at the low ranks
            c[:, 2] = np.abs(c[:, 2]) + 1
            c[:6, 2] = [0.0, -0.0, 0.0, -0.0, -0.0, 0.0]
        elif n == 1025:  # ties
            c[:, 2] = np.round(c[:, 2] * 64) / 64
        elif n == 4099:  # only negative z
            c[:, 2] = -np.abs(c[:, 2]) - 0.5
        elif n == 70001:
            # the ranks numpy interpolates, lo and lo + 1, sit on the two sides of a radix-digit
            # boundary: ranks 0 .. lo are the float below 1.0 (key 0xBF7FFFFF), the next three are 1.0
            # (key 0xBF800000), everything else is larger
            lo = int(np.floor(np.float32(np.float32(0.99) / np.float32(100)) * np.float32(n - 1)))
            z = (g.random(n) * 3 + 2).astype(np.float32)
            z[:lo + 1] = np.nextafter(np.float32(1), np.float32(0))
            z[lo + 1:lo + 4] = 1.0
            c[:, 2] = z[g.permutation(n)]
        clouds.append(c)
    return clouds


@pytest.mark.parametrize("columns", [6, 3])
def test_prepare_floor_is_host_floor(columns):
    _, SC, _ = _mods()
    clouds = _prepare_clouds(columns)
    store = SC.ScanStore(clouds, DEV, "scannet")  # one launch for the ten scans
    assert store.floor.dtype == np.float32 and store.floor.shape == (len(clouds),)
    for i, c in enumerate(clouds):
        want = SC.host_floor(c[:, 2])
        print("n = %d: floor %r, host %r" % (c.shape[0], store.floor[i], want))
        assert same_floor(store.floor[i], want), (c.shape[0], store.floor[i], want)
    assert store.floor[PREPARE_SIZES.index(102)] == 0
    assert store.floor[PREPARE_SIZES.index(4099)] < -0.5
    lo, hi = np.nextafter(np.float32(1), np.float32(0)), np.float32(1)
    assert lo <= store.floor[PREPARE_SIZES.index(70001)] <= hi
    assert torch.equal(store.dev["floor"].cpu(), torch.from_numpy(store.floor))


def test_prepare_names_the_scans_with_nonfinite_values():
    _, SC, _ = _mods()
    SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
    clouds = _prepare_clouds(6)
    clouds[3][17, 4] = np.nan       # a colour of scan 3
    clouds[8][4098, 2] = -np.inf    # the last z of scan 8
    with pytest.raises(SD.SceneError) as e:
        SC.ScanStore(clouds, DEV, "scannet")
    assert str(e.value).endswith(": scan0003 (1), scan0008 (1)")


# ------------------------------------------------------------------ scene_scan_batch_build
COUNTS = (1500, N, 5000)  # n below / equal / above N


def _indexed_clouds(dataset):
    """x is the point's own index, so a batch shows which points were picked"""
    _, SC, _ = _mods()
    clouds = SC.synthetic_clouds(len(COUNTS), max(COUNTS), seed=4, dataset=dataset)
    clouds = [c[:n].copy() for c, n in zip(clouds, COUNTS)]
    for c in clouds:
        c[:, 0] = np.arange(c.shape[0])
    return clouds


@pytest.fixture(scope="module", params=["scannet", "sunrgbd"])
def indexed_store(request):
    _, SC, _ = _mods()
    return SC.ScanStore(_indexed_clouds(request.param), DEV, request.param)


@pytest.mark.parametrize("use_color,use_height", [(c, h) for c in (False, True) for h in (False, True)])
def test_batch_build_is_host_batch(indexed_store, use_color, use_height):
    _, SC, _ = _mods()
    store = indexed_store
    loader = SC.ScanLoader(store, N, use_color=use_color, use_height=use_height, seed=11)
    g = np.random.default_rng(1)
    for B in (1, 3, 64):
        ids = (np.arange(B) + (2 if B == 1 else 0)) % len(COUNTS)
        counter = 100 + B
        got = loader.batch(ids, counter)
        want = loader.host_batch(ids, counter)
        pc = got["point_clouds"].cpu().numpy()
        assert pc.shape == (B, N, 3 + 3 * use_color + use_height) and pc.dtype == np.float32
        assert np.array_equal(bits(pc), bits(want["point_clouds"])), B
        assert np.array_equal(got["scan_idx"].cpu().numpy(), want["scan_idx"])
        for r, s in enumerate(ids):
            picks = pc[r, :, 0].astype(np.int64)
            assert picks.min() >= 0 and picks.max() < COUNTS[s]
            if COUNTS[s] >= N:
                assert len(np.unique(picks)) == N  # without replacement
        idx = np.stack([g.integers(0, COUNTS[s], N) for s in ids])
        got = loader.batch(ids, counter, draws={"idx": idx})["point_clouds"].cpu().numpy()
        want = loader.host_batch(ids, counter, draws={"idx": idx})["point_clouds"]
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(got[:, :, 0].astype(np.int64), idx)
    out = loader.allocate(3)
    again = loader.batch([0, 1, 2], 103, out=out)
    assert again["point_clouds"] is out["point_clouds"]
    assert np.array_equal(bits(out["point_clouds"].cpu().numpy()), bits(loader.host_batch([0, 1, 2], 103)["point_clouds"]))


@pytest.mark.parametrize("use_color,use_height", [(False, True), (True, True), (True, False)])
def test_batches_equal_the_labeled_loaders_eval_batches(tmp_path, use_color, use_height):
    V, SC, _ = _mods()
    SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
    names = ["scene%04d_00" % i for i in range(3)]
    for i, (name, n) in enumerate(zip(names, COUNTS)):
        SD.write_synthetic_scans(str(tmp_path), [name], num_points=n, instances=6, boxes=4, seed=30 + i)
    scenes = SD.ScanNetScenes(str(tmp_path), names, DEV, use_color=use_color, use_height=use_height)
    labeled = SD.ScanNetLoader(scenes, V.scannet_config(), N, seed=9)
    store = SC.ScanStore.from_files([str(tmp_path / (s + "_vert.npy")) for s in names], DEV, "scannet")
    loader = SC.ScanLoader(store, N, use_color=use_color, use_height=use_height, seed=9)
    for ids, counter in (([0, 1, 2], 0), ([2, 1], 6)):
        want = labeled.eval_batch(ids, counter)
        got = loader.batch(ids, counter)
        assert torch.equal(got["point_clouds"].view(torch.int32), want["point_clouds"].view(torch.int32))
        assert torch.equal(got["scan_idx"], want["scan_idx"])


# ------------------------------------------------------------------ scene_detections_pack
def _randomize_bn(module, seed):  # tests/test_inference_gpu.py's: folding matters
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


def _detector(tag, seed=0):
    V, _, _ = _mods()
    step = importlib.import_module("3dioumatch_amd.votenet.step")
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    det = step.build_detector(cfg, seed=seed).to(DEV)
    _randomize_bn(det, seed + 11)
    return det.eval(), cfg


def _config_dict(cfg, **over):
    cd = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
          "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False, "per_class_proposal": True,
          "conf_thresh": 0.05}
    cd.update(over)
    return cd


_END_POINTS = {}


def _end_points(tag):
    """the seeded detector's end points on three synthetic scenes, computed once per dataset; the
    first forty proposals of every scene share one objectness, so ties are ranked, and scene 0's
    objectness is pushed down: at the default threshold nothing of it is kept"""
    if tag not in _END_POINTS:
        I = importlib.import_module("3dioumatch_amd.votenet.inference")
        data = importlib.import_module("3dioumatch_amd.votenet.data")
        det, cfg = _detector(tag)
        pc = data.make_batch(3, 20000, cfg, seed=8, device=DEV)["point_clouds"]
        ep = I.InferenceEngine(det, graphs=False)(pc)
        ep["objectness_scores"][:, 0:40] = ep["objectness_scores"][:, 0:1].clone()
        ep["objectness_scores"][0, :, 1] -= 20.0
        ep["point_clouds"] = pc
        _END_POINTS[tag] = (ep, cfg)
    return _END_POINTS[tag]


def _assert_listing_equal(got, want):
    assert len(got) == len(want)
    for g_scene, w_scene in zip(got, want):
        assert len(g_scene) == len(w_scene)
        for (gc, gb, gs), (wc, wb, ws) in zip(g_scene, w_scene):
            assert gc == wc
            assert np.array_equal(bits(gb), bits(wb)) and bits(gs) == bits(ws)


PACK_CASES = [("scannet", dict(per_class_proposal=True)), ("scannet", dict(per_class_proposal=False)),
              ("scannet", dict(per_class_proposal=True, use_iou_for_nms=True)),
              ("scannet", dict(per_class_proposal=False, remove_empty_box=True)),
              ("scannet", dict(per_class_proposal=True, conf_thresh=2.0)),                   # keeps nothing
              ("scannet", dict(per_class_proposal=True, conf_thresh="median")),              # about half
              ("scannet", dict(per_class_proposal=False, conf_thresh=-1.0, nms_iou=1.5)),    # keeps everything
              ("sunrgbd", dict(per_class_proposal=True)), ("sunrgbd", dict(per_class_proposal=False)),
              ("sunrgbd", dict(per_class_proposal=True, use_iou_for_nms=True, conf_thresh=-1.0, nms_iou=1.5))]


@pytest.mark.parametrize("tag,over", PACK_CASES, ids=lambda v: v if isinstance(v, str) else
                         ",".join("%s=%s" % kv for kv in v.items()))
def test_pack_is_parse_predictions(tag, over):
    V, _, D = _mods()
    E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    ep, cfg = _end_points(tag)
    cd = _config_dict(cfg, **over)
    if over.get("conf_thresh") == "median":  # of the scenes whose objectness was left alone
        cd["conf_thresh"] = float(torch.softmax(ep["objectness_scores"][1:], -1)[:, :, 1].median())
    want = E.parse_predictions(dict(ep), cd)
    pred = E.parse_predictions_device(ep, cd)
    B, K = pred["keep"].shape
    S, first = B + 2, 1
    NC = cfg.num_class if cd["per_class_proposal"] else 0
    arena = torch.full((D.arena_layout(S, K, NC)[1],), 7.0, dtype=torch.float32, device=DEV)
    out = D.pack_end_points(arena, S, first, ep, cd)
    assert out[0] is arena and out[1:] == (K, NC, B)
    found = D.Detections(arena, ["s%d" % i for i in range(S)], K, NC, cfg.num_class)
    _assert_listing_equal(found.as_map_cls()[first:first + B], want)

    planes = found.planes()
    keep = pred["keep"].cpu().numpy()
    obj = torch.softmax(ep["objectness_scores"], -1)[:, :, 1].cpu().numpy()
    size64, heading64 = E.decode_boxes(ep, cfg)
    box = torch.cat([ep["center"], size64.float(), heading64.float().unsqueeze(-1)], -1).cpu().numpy()
    counts = planes["count"][first:first + B]
    print("kept per scene:", counts.tolist(), "of", K)
    assert counts.tolist() == keep.sum(1).tolist()
    if over.get("conf_thresh") == 2.0:
        assert not counts.any()
    if "conf_thresh" not in over:  # one threshold: nothing of scene 0, something of the others
        assert counts[0] == 0 and counts[1:].all()
    if over.get("conf_thresh") == "median":
        assert counts[0] == 0 and (counts[1:] > 0).all() and (counts[1:] < K).all()
    if over.get("nms_iou") == 1.5:
        assert (counts == K).all()
    for b in range(B):
        s, c = first + b, int(counts[b])
        order = sorted(np.nonzero(keep[b])[0].tolist(), key=lambda j: (-float(obj[b, j]), j))
        assert planes["proposal"][s, :c].tolist() == order  # objectness descending, then proposal
        assert np.array_equal(bits(planes["box"][s, :c]), bits(box[b, order]))
        assert np.array_equal(planes["cls"][s, :c], pred["cls"][b].cpu().numpy()[order])
        for name in ("proposal", "cls", "score", "box", "corners"):
            assert not planes[name][s, c:].view(np.uint32).any(), name  # rows past count: zero bits
    if over.get("nms_iou") == 1.5:  # the tie group of forty is all there, in proposal order
        p = planes["proposal"][first].tolist()
        at = p.index(0)
        assert p[at:at + 40] == list(range(40))
    # the rows of other scans are not touched
    for name in planes:
        for s in (0, S - 1):
            assert (planes[name][s].view(np.uint32) == np.float32(7).view(np.uint32)).all(), name


# ------------------------------------------------------------------ detect(), end to end
@pytest.fixture(scope="module")
def run_setup():
    V, SC, D = _mods()
    I = importlib.import_module("3dioumatch_amd.votenet.inference")
    det, cfg = _detector("scannet")
    store = SC.ScanStore(SC.synthetic_clouds(6, 25000, seed=3, color=False), DEV, "scannet")
    loader = SC.ScanLoader(store, 20000, seed=2)
    engine = I.InferenceEngine(det)
    # a confidence threshold in the middle of this detector's objectness: about half is kept
    ep = engine(loader.batch([0, 1], 0)["point_clouds"])
    thresh = float(torch.softmax(ep["objectness_scores"], -1)[:, :, 1].median())
    return engine, loader, cfg, thresh


def _listing_by_hand(engine, loader, cd, counter, opt_step=0, opt_rate=5e-4):
    E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    O = importlib.import_module("3dioumatch_amd.votenet.iou_opt")
    batches = [b["point_clouds"] for b in loader.batches(4, counter)]
    assert [b.shape[0] for b in batches] == [4, 2]
    listing = []
    for pc, ep in zip(batches, engine.run(batches)):
        if opt_step > 0:
            ep = O.optimize_boxes(engine.detector, ep, opt_rate, opt_step)
        ep.setdefault("point_clouds", pc)
        listing += E.parse_predictions(ep, cd)
    return listing


@pytest.mark.parametrize("opt_step", [0, 2])
def test_detect_is_engine_run_and_parse_predictions(run_setup, opt_step):
    V, _, D = _mods()
    engine, loader, cfg, thresh = run_setup
    cd = _config_dict(cfg, per_class_proposal=True, conf_thresh=thresh)
    want = _listing_by_hand(engine, loader, cd, counter=5, opt_step=opt_step, opt_rate=1e-3)
    found = V.detect(engine, loader, cd, batch_size=4, opt_step=opt_step, opt_rate=1e-3, counter=5)
    assert isinstance(found, D.Detections) and len(found) == 6
    assert found.names == loader.store.names
    _assert_listing_equal(found.as_map_cls(), want)
    counts = found.planes()["count"]
    print("kept per scan:", counts.tolist())
    assert counts.sum() > 0 and (counts < found.K).any()
    assert found.by_name("scan0005")["count"] == found[5]["count"]


def test_detect_is_reproducible_and_its_loop_does_not_synchronise(run_setup):
    V, _, D = _mods()
    engine, loader, cfg, thresh = run_setup
    cd = _config_dict(cfg, per_class_proposal=False, conf_thresh=thresh)
    first = V.detect(engine, loader, cd, batch_size=4, counter=1)  # warm-up: graphs captured
    V.detect(engine, loader, cd, batch_size=4, counter=1, opt_step=2)
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
        second = V.detect(engine, loader, cd, batch_size=4, counter=1)   # raises nothing
        V.detect(engine, loader, cd, batch_size=4, counter=1, opt_step=2)  # nor with the box optimisation
        with pytest.raises(RuntimeError):
            second[0]   # reading is the first synchronising call
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert torch.equal(first.arena.view(torch.int32), second.arena.view(torch.int32))
    assert second[0]["count"] == first[0]["count"]


# ------------------------------------------------------------------ poisoned allocations
@pytest.mark.parametrize("fill", dirty_memory.FILLS, ids=dirty_memory.FILL_IDS)
def test_bindings_on_poisoned_allocations(fill):
    V, SC, D = _mods()
    E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    store = SC.ScanStore(_indexed_clouds("scannet"), DEV, "scannet")
    d = store.dev
    loader = SC.ScanLoader(store, N, use_color=True, use_height=True, seed=1)
    ep, cfg = _end_points("scannet")
    cd = _config_dict(cfg, per_class_proposal=True)
    pred = E.parse_predictions_device(ep, cd)
    size64, heading64 = E.decode_boxes(ep, cfg)
    obj = torch.softmax(ep["objectness_scores"], -1)[:, :, 1]
    B, K = pred["keep"].shape

    def run():
        floor, bad = SC.scan_prepare_gpu(d["cloud"], d["offset"], d["count"])
        pc = loader.batch([0, 1, 2], 4)["point_clouds"]
        arena = D.new_arena(B, K, cfg.num_class, DEV)
        D.pack_gpu(arena, B, 0, pred["keep"], obj, pred["cls"], pred["score"], ep["center"], size64, heading64,
                   pred["corners"])
        torch.cuda.synchronize()
        return floor, bad, pc, arena

    clean = run()
    with dirty_memory.poisoned(fill) as p:
        dirty = run()
    assert p.count >= 3  # floor, point_clouds, arena
    for name, c, x in zip(("floor", "nonfinite", "point_clouds", "arena"), clean, dirty):
        assert torch.equal(c.view(torch.int32), x.view(torch.int32)), name
