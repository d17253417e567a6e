"""GPU tests of the SUN RGB-D batch builder (csrc/sunrgbd_batch.hip through votenet/sunrgbd_data.py):
explicit draws against the reference's own datasets (tests/golden/sunrgbd_data_ref.npz, with the
bounds of test_sunrgbd_data.py), device draws against the host restatement, repeatability, train
steps fed by the side-stream loop, and evaluation of a SUN RGB-D store."""
import importlib
import math

import numpy as np
import pytest
import torch

from conftest import load_pkg
from test_sunrgbd_data import (GOLD, SCENES, VARIANTS, batch_args, compare_to_golden, golden_draws,
                               loader_for, within_ulp)

load_pkg()
SD = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
V = importlib.import_module("3dioumatch_amd.votenet")
DEV = torch.device("cuda", 0)
pytestmark = pytest.mark.gpu


def host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items() if torch.is_tensor(v)}


def assert_batches_match(got, want):
    """The device's batch against the host restatement of the same draws: both read the same float32
    store, so every float is within 1 float32 ulp (cos / sin of the two maths libraries, BLAS's
    fused products), heading residuals within 3e-8 and votes within 2e-6 as against the reference."""
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if k == "vote_label":
            np.testing.assert_allclose(g, w, rtol=0, atol=2e-6, err_msg=k)
        elif k == "heading_residual_label":
            np.testing.assert_allclose(g, w, rtol=0, atol=3e-8, err_msg=k)
        elif g.dtype.kind == "f":
            within_ulp(g, w, key=k)
        else:
            assert np.array_equal(g, w), k


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_explicit_draws_reproduce_the_reference(tmp_path, variant):
    _, use_color, unl_row, labels = VARIANTS[variant]
    loader = loader_for(tmp_path, use_color, DEV)
    report = {}
    for i, s in enumerate(SCENES):
        kind, (lab, unl), labels = batch_args(variant, i)
        b = loader._build(kind, lab, unl, 0, labels, draws=golden_draws(variant, s))
        compare_to_golden(host(b), variant, s, report)
    print(variant, "largest |error| per key:", {k: "%.3g" % v for k, v in sorted(report.items())})


def _synthetic_loader(tmp_path, num_points=3000, seed=11, use_color=False):
    names = ["%06d" % i for i in range(1, 7)]
    SD.write_synthetic_scans(str(tmp_path), names[:5], num_points=4000, boxes=10, seed=1)
    SD.write_synthetic_scans(str(tmp_path), names[5:], num_points=2500, boxes=0, seed=2, dtype=np.float64)
    scenes = SD.SunRgbdScenes(str(tmp_path), names, DEV, use_color=use_color, use_height=True)
    cfg = V.sunrgbd_config(mean_size_arr=GOLD["mean_size"])
    return SD.SunRgbdLoader(scenes, cfg, num_points, seed=seed, labeled=names[:3], unlabeled=names[3:])


@pytest.mark.parametrize("use_color", [False, True])
def test_device_draws_equal_the_host_restatement(tmp_path, use_color):
    loader = _synthetic_loader(tmp_path, use_color=use_color)
    for counter in (0, 7):
        for labels in (True, False):
            dev = host(loader.semi_batch([0, 2], [2, 0, 1], counter, unlabeled_labels=labels))
            want = loader.host_batch("semi", [0, 2], [2, 0, 1], counter, unlabeled_labels=labels)
            assert_batches_match(dev, want)
        assert_batches_match(host(loader.pretrain_batch([1, 2], counter)),
                             loader.host_batch("pretrain", [1, 2], None, counter))
        assert_batches_match(host(loader.eval_batch([0, 1, 2], counter)),
                             loader.host_batch("eval", [0, 1, 2], None, counter))


def test_colour_pretrain_batch_equals_the_restatement(tmp_path):
    """The per-point colour augmentation with the device's own draws (keyed by the source point):
    brightness, shift, jitter, clip and the 30 % drop all take part."""
    loader = _synthetic_loader(tmp_path, use_color=True)
    dev = host(loader.pretrain_batch([0, 1, 2], 5))
    want = loader.host_batch("pretrain", [0, 1, 2], None, 5)
    assert_batches_match(dev, want)
    rgb = dev["point_clouds"][:, :, 3:6]
    dropped = (rgb == -0.5).all(-1).mean()
    assert 0.25 < dropped < 0.35, dropped
    plain = loader.host_batch("eval", [0, 1, 2], None, 5)["point_clouds"][:, :, 3:6]
    assert not np.array_equal(np.sort(rgb.reshape(-1)), np.sort(plain.reshape(-1)))


def test_same_counter_same_bits_other_counter_other_batch(tmp_path):
    loader = _synthetic_loader(tmp_path, use_color=True)
    a = host(loader.semi_batch([0, 1], [0, 2], 3))
    b = host(loader.semi_batch([0, 1], [0, 2], 3))
    c = host(loader.semi_batch([0, 1], [0, 2], 4))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["point_clouds"], c["point_clouds"])
    assert not np.array_equal(a["ema_point_clouds"], c["ema_point_clouds"])
    assert not np.array_equal(a["vote_label"], c["vote_label"])
    p = host(loader.pretrain_batch([0, 1], 3))
    q = host(loader.pretrain_batch([0, 1], 3))
    for k in p:
        assert np.array_equal(p[k], q[k]), k


def _plan(kind, steps):
    """`steps` batches over consecutive epochs (3 labeled scenes, 2 per batch: one batch an epoch)."""
    plan = []
    for e in range(steps):
        if kind == "semi":
            plan += list(SD.epoch_plan(3, 2, e, seed=1, num_unlabeled=3, unlabeled_batch_size=2))
        else:
            plan += list(SD.epoch_plan(3, 2, e, seed=1))
    return plan[:steps]


def _step_cls(kind):
    return (V.SemiSupervisedStep, 2e-3) if kind == "semi" else (V.SupervisedStep, 1e-3)


def _snapshot(loss, runner):
    return (loss.detach().clone(), runner.flat_grad.detach().clone(), runner.flat_params.detach().clone())


@pytest.mark.parametrize("kind", ["pretrain", "semi"])
def test_fed_steps_equal_steps_on_independently_built_batches(tmp_path, kind):
    """Three graph-mode steps fed by the side-stream loop, with no host synchronisation inside the
    loop, equal (loss, gradient, parameters: bit for bit) three steps of a second runner fed with
    the same (counter, ids) built afterwards on their own and sent through host memory."""
    loader = _synthetic_loader(tmp_path)
    plan = _plan(kind, 3)
    cls, lr = _step_cls(kind)

    runner = cls(loader.config, DEV, world_size=1, num_proposal=64, seed=3, graphs=True, lr=lr)
    torch.manual_seed(9)
    torch.cuda.manual_seed_all(9)
    fed = [_snapshot(runner(b)[0], runner) for b in SD.feed(runner, loader, plan, kind=kind)]
    torch.cuda.synchronize()
    assert runner.graphs and len(fed) == 3

    copies = []
    for counter, lab, unl in plan:
        b = loader._build(kind, lab, unl, counter)
        copies.append({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.items()})
    runner = cls(loader.config, DEV, world_size=1, num_proposal=64, seed=3, graphs=True, lr=lr)
    torch.manual_seed(9)
    torch.cuda.manual_seed_all(9)
    views = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()} for c in copies]
    runner.prefetch_geometry(views[0])
    again = []
    for i, v in enumerate(views):
        if i + 1 < len(views):
            runner.prefetch_geometry(views[i + 1])
        again.append(_snapshot(runner(v)[0], runner))
    torch.cuda.synchronize()
    for i, ((l0, g0, p0), (l1, g1, p1)) in enumerate(zip(fed, again)):
        assert bool(torch.isfinite(l0)), i
        assert torch.equal(l0, l1), (i, float(l0), float(l1))
        assert torch.equal(g0, g1), i
        assert torch.equal(p0, p1), i


@pytest.mark.parametrize("kind", ["pretrain", "semi"])
def test_eager_runner_fed_without_host_syncs(tmp_path, kind):
    """An eager runner (graphs=False: its backward frees activations the GPU is still using) fed
    for five steps with no host synchronisation: every yielded batch, cloned on the main stream
    right when it is yielded, equals the host restatement of its (counter, ids) -- no build wrote
    into memory a step still used, and no step wrote into a set -- and every loss is finite."""
    loader = _synthetic_loader(tmp_path)
    plan = _plan(kind, 5)
    cls, lr = _step_cls(kind)
    runner = cls(loader.config, DEV, world_size=1, num_proposal=64, seed=3, graphs=False, lr=lr)
    seen, losses = [], []
    for b in SD.feed(runner, loader, plan, kind=kind):
        seen.append({k: v.clone() for k, v in b.items() if torch.is_tensor(v)})
        loss, _ = runner(b)
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    assert not runner.graphs and len(seen) == 5
    assert bool(torch.isfinite(torch.stack(losses)).all())
    for (counter, lab, unl), got in zip(plan, seen):
        assert_batches_match(host(got), loader.host_batch(kind, lab, unl, counter))


def test_explicit_draws_out_of_range_are_refused_on_the_device_path(tmp_path):
    loader = _synthetic_loader(tmp_path)
    n = int(loader.scenes.count[loader.labeled[0]])
    u = np.full((1, 3), 0.75)
    bad = np.arange(loader.num_points, dtype=np.int64)[None] % n
    bad[0, -1] = n
    with pytest.raises(ValueError, match="'idx' out of range"):
        loader.pretrain_batch([0], draws={"idx": bad, "u": u})
    bad[0, -1] = n - 1
    draws = {"idx": bad, "u": u}
    assert_batches_match(host(loader.pretrain_batch([0], draws=draws)),
                         loader.host_batch("pretrain", [0], None, draws=draws))


def test_evaluate_on_eval_batches_of_a_sunrgbd_store(tmp_path):
    I = importlib.import_module("3dioumatch_amd.votenet.inference")  # noqa: E741
    step = importlib.import_module("3dioumatch_amd.votenet.step")
    names = ["%06d" % i for i in range(1, 6)]
    SD.write_synthetic_scans(str(tmp_path), names, num_points=25000, boxes=30, seed=6)
    scenes = SD.SunRgbdScenes(str(tmp_path), names, DEV, use_color=False, use_height=True)
    assert set(scenes.boxes[:4, :30, 7].astype(int).reshape(-1).tolist()) == set(range(10))
    cfg = V.sunrgbd_config(mean_size_arr=GOLD["mean_size"])
    loader = SD.SunRgbdLoader(scenes, cfg, 20000, seed=1)
    det = step.build_detector(cfg, seed=0).to(DEV).eval()
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
                   "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
                   "per_class_proposal": True, "conf_thresh": 0.05}
    batches = list(SD.eval_batches(loader, 2))
    assert [b["point_clouds"].shape[0] for b in batches] == [2, 2, 1]
    assert_batches_match(host(batches[2]), loader.host_batch("eval", [4], None, 2))
    got = I.evaluate(I.InferenceEngine(det), batches[:2], config_dict, opt_step=0)
    assert len(got) == 2
    for metrics in got:
        assert math.isfinite(metrics["mAP"]) and math.isfinite(metrics["AR"]), metrics
