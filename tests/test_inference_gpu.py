"""The inference engine on the MI355X: the one-pass eval kernels of the pooled shared MLPs
(csrc/mlp_eval_pool.hip) against float64 torch, the engine (votenet/inference.py) against the plain
eval forward, its statelessness, graph replay and pipelining, and inference.evaluate against
iou_opt.evaluate.

The ball query of vote aggregation runs on PREDICTED vote coordinates: two correct fp32 forwards may
put a different point into a few balls, so the engine comparison counts the proposals that disagree
instead of loosening the tolerance for all of them (as test_iou_opt_gpu.py does)."""
import importlib
import math

import pytest
import torch

import eval_pool_cases
from conftest import load_pkg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _mods():
    load_pkg()
    return (importlib.import_module("pointnet2.pytorch_utils"),
            importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.inference"),
            importlib.import_module("3dioumatch_amd.votenet.step"),
            importlib.import_module("3dioumatch_amd.votenet.data"))


def _randomize_bn(module, seed):
    """non-trivial running statistics and some negative gammas, so that folding matters"""
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


def _mlp(U, chans, seed):
    torch.manual_seed(seed)
    mlp = U.SharedMLP(chans, bn=True)
    _randomize_bn(mlp, seed)
    return mlp.to(DEV).eval()


def _ref(mlp, x, dtype):
    y = x.to(dtype)
    for layer in mlp:
        w = layer.conv.weight.to(dtype).reshape(layer.conv.weight.shape[0], -1)
        bn = next(layer.bn.children())
        y = torch.einsum("ok,bkmn->bomn", w, y)
        scale = bn.weight.to(dtype) / torch.sqrt(bn.running_var.to(dtype) + bn.eps)
        shift = bn.bias.to(dtype) - bn.running_mean.to(dtype) * scale
        y = torch.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    return y.amax(3)


def _ref_f64(mlp, x):
    return _ref(mlp, x, torch.float64)


def _fused(U, mlp, x):
    plan = U.EvalPlan(mlp)
    with torch.no_grad(), U.fused_eval({id(mlp): plan}):
        out = mlp.forward_pooled(x)
    torch.cuda.synchronize()
    return out, plan.hits


def _fp32_grade(got, mlp, x):
    """tests/test_eval_pool_gpu.py's bound: the error against float64 is at most RATIO times that of the
    same module in fp32 torch ops on the same data (no absolute floor)"""
    want = _ref_f64(mlp, x)
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        plain = _ref(mlp, x, torch.float32)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old
    e_got, e_plain = eval_pool_cases.rel_err(got, want), eval_pool_cases.rel_err(plain, want)
    print("e(fused) %.3e  e(plain_fp32) %.3e" % (e_got, e_plain))
    assert e_got <= eval_pool_cases.RATIO * e_plain, (e_got, e_plain)


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("ns", [16, 32, 64])
@pytest.mark.parametrize("m", [2048, 1000])
def test_lin4_form_matches_float64(b, ns, m):
    U, _, _, _, _ = _mods()
    K = importlib.import_module("pointnet2._mlp_ext")
    mlp = _mlp(U, [4, 64, 64, 128], seed=ns + m)
    x = torch.randn(b, 4, m, ns, device=DEV)
    out, hits = _fused(U, mlp, x)
    assert hits == int(K.eval_lin4_supported(b, 4, 64, 128, m, ns))  # else: the plain path served it
    assert hits == 1 or m == 1000
    _fp32_grade(out, mlp, x)


@pytest.mark.parametrize("c_out,m,ns,covered", [
    (256, 1024, 32, True),   # SA2
    (256, 512, 16, True),    # SA3
    (256, 256, 16, True),    # SA4
    (128, 256, 16, True),    # vote aggregation
    (128, 256, 64, True),    # GridConv / IoU branch
    (128, 256, 8, False),    # outside the gate: the plain path
])
def test_stored_form_matches_float64(c_out, m, ns, covered):
    U, _, _, _, _ = _mods()
    mlp = _mlp(U, [131, 128, 128, c_out], seed=c_out + m + ns)
    x = torch.randn(2, 131, m, ns, device=DEV)
    out, hits = _fused(U, mlp, x)
    assert hits == int(covered)
    _fp32_grade(out, mlp, x)


def _detector(V, step, tag, seed=0):
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    det = step.build_detector(cfg, seed=seed).to(DEV)
    _randomize_bn(det, seed + 11)
    return det.eval(), cfg


def _compare_end_points(got, want, k, max_bad=0.02):
    """every float key within 1e-4 of its range; proposal-indexed keys may disagree on a few proposals"""
    assert set(got) == set(want)
    b = want["center"].shape[0]
    bad = torch.zeros(b, k, dtype=torch.bool, device=DEV)
    for key, w in want.items():
        g = got[key]
        if not torch.is_tensor(w):
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, key
        if not w.is_floating_point():
            if w.dim() >= 2 and w.shape[1] == k:
                bad |= (g != w).reshape(b, k, -1).any(-1)
            else:
                assert torch.equal(g, w), key
            continue
        tol = 1e-4 * max(w.abs().max().item(), 1e-6)
        off = (g - w).abs() > tol
        if w.dim() >= 2 and w.shape[1] == k:
            bad |= off.reshape(b, k, -1).any(-1)
        elif w.dim() == 3 and w.shape[2] == k:
            bad |= off.any(1)
        else:
            assert not off.any(), "%s: max error %.3e" % (key, (g - w).abs().max().item())
    n_bad = int(bad.sum().item())
    assert n_bad <= max(2, int(max_bad * b * k)), "%d of %d proposals disagree" % (n_bad, b * k)
    return n_bad


@pytest.mark.parametrize("tag,b,n", [("scannet", 8, 40000), ("sunrgbd", 16, 20000)])
def test_engine_matches_plain_eval_forward(tag, b, n):
    U, V, I, step, data = _mods()
    det, cfg = _detector(V, step, tag)
    pc = data.make_batch(b, n, cfg, seed=3, device=DEV)["point_clouds"]
    with torch.no_grad():
        want = det({"point_clouds": pc})
    engine = I.InferenceEngine(det)
    got = engine(pc)
    torch.cuda.synchronize()
    # all six pooled call sites went through the one-pass kernels
    assert sum(1 for plan in engine.plans.values() if plan.hits > 0) == 6
    _compare_end_points(got, want, det.num_proposal)


def test_engine_changes_no_state_and_follows_refresh():
    U, V, I, step, data = _mods()
    det, cfg = _detector(V, step, "scannet")
    state = {k: v.clone() for k, v in det.state_dict().items()}
    engine = I.InferenceEngine(det)
    for s in range(3):
        engine(data.make_batch(8, 40000, cfg, seed=s, device=DEV)["point_clouds"])
    torch.cuda.synchronize()
    after = det.state_dict()
    for k, v in state.items():
        assert torch.equal(v, after[k]), k
    other, _ = _detector(V, step, "scannet", seed=5)
    det.load_state_dict(other.state_dict())
    engine.refresh()
    pc = data.make_batch(8, 40000, cfg, seed=9, device=DEV)["point_clouds"]
    with torch.no_grad():
        want = det({"point_clouds": pc})
    _compare_end_points(engine(pc), want, det.num_proposal)


def test_replay_and_pipelining_are_bit_exact():
    U, V, I, step, data = _mods()
    det, cfg = _detector(V, step, "scannet")
    clouds = [data.make_batch(8, 40000, cfg, seed=20 + s, device=DEV)["point_clouds"] for s in range(4)]
    eager = I.InferenceEngine(det, graphs=False)
    graphed = I.InferenceEngine(det)
    alone = [eager(pc) for pc in clouds]
    replayed = graphed(clouds[0])  # captures, then replays
    replayed2 = graphed(clouds[0])
    piped = list(graphed.run(clouds))
    torch.cuda.synchronize()
    assert len(piped) == 4
    for key, v in alone[0].items():
        if torch.is_tensor(v):
            assert torch.equal(replayed[key], v), key
            assert torch.equal(replayed2[key], v), key
    for i in range(4):
        for key, v in alone[i].items():
            if torch.is_tensor(v):
                assert torch.equal(piped[i][key], v), (i, key)
    assert not torch.equal(piped[0]["center"], piped[1]["center"])  # distinct batches


def test_evaluate_matches_iou_opt_evaluate():
    U, V, I, step, data = _mods()
    O = importlib.import_module("3dioumatch_amd.votenet.iou_opt")
    det, cfg = _detector(V, step, "scannet")
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
                   "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
                   "per_class_proposal": True, "conf_thresh": 0.05}
    batches = [data.make_batch(4, 20000, cfg, seed=40 + s, device=DEV) for s in range(2)]
    engine = I.InferenceEngine(det)
    want = O.evaluate(det, batches, config_dict, opt_step=0)
    got = I.evaluate(engine, batches, config_dict, opt_step=0)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key, val in w.items():
            if isinstance(val, float) and not (math.isnan(val) and math.isnan(g[key])):  # (no such class)
                assert abs(g[key] - val) <= 1e-3, (key, g[key], val)
    got2 = I.evaluate(engine, batches, config_dict, opt_step=2, opt_rate=1e-3)
    want2 = O.evaluate(det, batches, config_dict, opt_step=2, opt_rate=1e-3)
    for g, w in zip(got2, want2):
        assert set(g) == set(w)
        assert math.isnan(g["mAP"]) == math.isnan(w["mAP"])
        if not math.isnan(w["mAP"]):
            assert abs(g["mAP"] - w["mAP"]) <= 5e-2
