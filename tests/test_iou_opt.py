"""Test-time IoU optimisation (votenet/iou_opt.py) on the CPU: the autograd engine against the
REFERENCE's GridConv driven by the loop of train.py:444-491 (tests/golden/make_iou_opt_golden.py,
float64, oracle stand-in for three_nn), and evaluate() against the hand-called evaluation chain."""
import importlib
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, load_pkg


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.iou_opt"))


@pytest.fixture()
def standin(oracle):
    load_pkg()
    utils = importlib.import_module("pointnet2.pointnet2_utils")
    from oracle import standin as oracle_ext
    real = utils._ext
    utils._ext = oracle_ext.make(oracle)
    yield
    utils._ext = real


def _detector(V, cfg, k, seed_feat_dim=256):
    det = V.VoteNet(cfg.num_class, cfg.num_heading_bin, cfg.num_size_cluster, cfg.mean_size_arr, cfg,
                    input_feature_dim=1, num_proposal=k, sampling="seed_fps")
    heads = importlib.import_module("3dioumatch_amd.votenet.heads")
    det.grid_conv = heads.GridConv(cfg.num_class, cfg.num_heading_bin, cfg.num_size_cluster,
                                   cfg.mean_size_arr, k, "seed_fps", seed_feat_dim=seed_feat_dim)
    return det


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_autograd_engine_matches_reference_loop(tag, standin):
    V, O = _mods()
    sys.path.insert(0, GOLDEN)
    try:
        from make_iou_opt_golden import seeded_state
    finally:
        sys.path.remove(GOLDEN)
    g = golden("iou_opt_ref.npz")
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    inp = {k.split("/", 2)[2]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag + "/in/")}
    b, k = inp["center"].shape[:2]
    det = _detector(V, cfg, k, seed_feat_dim=inp["seed_features"].shape[1]).double().eval()
    assert sorted(det.grid_conv.state_dict()) == g[tag + "/weight_keys"].tolist()
    seeded_state(det.grid_conv, int(g[tag + "/weight_seed"]))
    # GridConv's unit grid is made in float32 (+-1/3 rounded); the float64 reference's is not
    step = torch.linspace(-1, 1, 4, dtype=torch.float64)
    det.grid_conv.__dict__["_unit_cache"] = {
        "cpu": torch.stack(torch.meshgrid(step, step, step, indexing="ij"), -1).view(64, 3)}
    opt_step = g[tag + "/center"].shape[0] - 1
    rate = float(g[tag + "/opt_rate"])

    trace = []
    O._optimize_autograd(det, inp, rate, opt_step, trace)
    assert len(trace) == opt_step + 1  # opt_step + 1 updates
    for i, (c, s, iou) in enumerate(trace):
        np.testing.assert_allclose(c.numpy(), g[tag + "/center"][i], rtol=0, atol=1e-9)
        np.testing.assert_allclose(s.numpy(), g[tag + "/size"][i], rtol=0, atol=1e-9)
        np.testing.assert_allclose(iou.numpy(), g[tag + "/iou"][i], rtol=0, atol=1e-9)
    # the boxes really moved
    assert np.abs(g[tag + "/center"][-1] - inp["center"].numpy()).max() > 1e-3

    ep = dict(inp, heading_scores=torch.zeros(b, k, cfg.num_heading_bin), marker=torch.ones(1))
    out = O.optimize_boxes(det, ep, rate, opt_step, engine="autograd")
    np.testing.assert_allclose(out["center"].numpy(), g[tag + "/center"][-1], rtol=0, atol=1e-9)
    np.testing.assert_allclose(out["iou_scores"].numpy(), g[tag + "/iou"][-1], rtol=0, atol=1e-9)
    assert out["size_residuals"].shape == (b, k, cfg.num_size_cluster, 3)
    np.testing.assert_allclose(out["size_residuals"].numpy(), g[tag + "/size_residuals"], rtol=0, atol=1e-9)
    for key in ("size", "heading", "heading_scores", "marker", "seed_xyz", "sem_cls_scores"):
        assert out[key] is ep[key]  # everything else unchanged
    assert "iou_scores" not in ep and ep["center"] is inp["center"]  # the input dict is not modified
    with pytest.raises(ValueError):
        O.optimize_boxes(det, ep, rate, opt_step, engine="nope")


def test_optimize_boxes_rejects_training_mode_and_class_free_iou(standin):
    V, O = _mods()
    cfg = V.scannet_config()
    det = _detector(V, cfg, 8, seed_feat_dim=16)
    ep = {"center": torch.zeros(1, 8, 3)}
    with pytest.raises(ValueError, match="eval mode"):
        O.optimize_boxes(det.train(), ep, 1e-3, 2)
    heads = importlib.import_module("3dioumatch_amd.votenet.heads")
    det.grid_conv = heads.GridConv(cfg.num_class, cfg.num_heading_bin, cfg.num_size_cluster,
                                   cfg.mean_size_arr, 8, "seed_fps", seed_feat_dim=16,
                                   iou_class_depend=False)
    with pytest.raises(ValueError, match="iou_class_depend"):
        O.optimize_boxes(det.eval(), ep, 1e-3, 2)
    with pytest.raises(ValueError):
        O.evaluate(det.eval(), [], {"dataset_config": cfg}, opt_step=3)
    with pytest.raises(ValueError):
        O.evaluate(det.train(), [], {"dataset_config": cfg})


class _Replay(torch.nn.Module):
    """a detector stand-in whose eval forward returns fixed head outputs"""

    def __init__(self, outputs):
        super().__init__()
        self.outputs = outputs

    def forward(self, inputs):
        return dict(self.outputs[int(inputs["point_clouds"][0, 0, 0])])


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_evaluate_without_optimisation_is_the_plain_chain(tag, oracle, monkeypatch):
    V, O = _mods()
    D = importlib.import_module("3dioumatch_amd.votenet.eval_det")
    E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    from test_eval_helper import _oracle_nms
    from test_eval_det import _oracle_best_match, _perfect_end_points
    monkeypatch.setattr(E, "_nms3d", _oracle_nms(oracle))
    monkeypatch.setattr(D, "_best_match", _oracle_best_match(oracle))
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
                   "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
                   "per_class_proposal": True, "conf_thresh": 0.05}
    rng = np.random.default_rng(5)
    outputs, batches = [], []
    for i in range(2):
        ep = _perfect_end_points(V, cfg, rng)
        # perturb the head so that AP is not trivially 1
        ep["center"] = ep["center"] + torch.from_numpy(rng.normal(0, 0.15, tuple(ep["center"].shape))).float()
        labels = {key: val for key, val in ep.items() if key.endswith("_label") or key.endswith("_mask")}
        head = {key: val for key, val in ep.items() if key not in labels and key != "point_clouds"}
        outputs.append(head)
        batches.append(dict(labels, point_clouds=torch.full((3, 4, 3), float(i))))
    det = _Replay(outputs).eval()
    got = O.evaluate(det, batches, config_dict, opt_step=0, ap_iou_thresholds=(0.25, 0.5))

    calcs = [V.APCalculator(t, None) for t in (0.25, 0.5)]
    for i, batch in enumerate(batches):
        ep = dict(outputs[i])
        ep.update({key: val for key, val in batch.items() if key != "point_clouds"})
        ep["point_clouds"] = batch["point_clouds"]
        pred = V.parse_predictions(ep, config_dict)
        gt = V.parse_groundtruths(ep, config_dict)
        for calc in calcs:
            calc.step(pred, gt)
    want = [calc.compute_metrics() for calc in calcs]
    assert len(got) == 2
    for a, b in zip(got, want):
        assert a.keys() == b.keys()
        for key in a:
            assert a[key] == b[key] or (np.isnan(a[key]) and np.isnan(b[key])), key
    aps = [v for key, v in got[0].items() if key.endswith("Average Precision") and not np.isnan(v)]
    assert aps and 0.0 < np.mean(aps) < 1.0
