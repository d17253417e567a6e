"""Test-time IoU optimisation on the MI355X: the box-gradient kernel (votenet_iou_opt_box_step)
against a float64 autograd of its formula, and the device engine of votenet/iou_opt.py against
the autograd engine (the reference loop, train.py:444-491) from common points.

The three nearest seeds and the max-pool arg-max are discontinuous: two correct fp32 forwards
may pick a different neighbour or arg-max for a few grid points, so the engine comparisons count
the boxes that disagree instead of loosening the tolerance for all of them."""
import importlib

import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu


def _mods():
    load_pkg()
    return (importlib.import_module("3dioumatch_amd.votenet"),
            importlib.import_module("3dioumatch_amd.votenet.iou_opt"),
            importlib.import_module("3dioumatch_amd._lib"))


def _unit(dev, dtype=torch.float32):
    step = torch.linspace(-1, 1, 4, device=dev, dtype=dtype)
    return torch.stack(torch.meshgrid(step, step, step, indexing="ij"), -1).view(64, 3).contiguous()


def _formula_f64(unit, seed_xyz, idx, proj, w0xyz, dy0, center, size, heading):
    """dL/d(center, size) of the kernel's formula by float64 autograd (a_j and W0[:, :3]^T dy0 are
    constants of the pass: they do not depend on the box)"""
    b, k = heading.shape
    c = center.double().clone().requires_grad_(True)
    s = size.double().clone().requires_grad_(True)
    u = unit.double().view(1, 1, 64, 3)
    loc = u * s.unsqueeze(2)
    cos, sin = torch.cos(heading.double()).view(b, k, 1), torch.sin(heading.double()).view(b, k, 1)
    rel = torch.stack([loc[..., 0] * cos + loc[..., 1] * sin, loc[..., 1] * cos - loc[..., 0] * sin,
                       loc[..., 2]], -1)
    q = (rel + c.unsqueeze(2)).view(b, k * 64, 1, 3)
    il = idx.long()
    p = torch.gather(seed_xyz.double(), 1, il.view(b, -1, 1).expand(-1, -1, 3)).view(b, k * 64, 3, 3)
    d = torch.sqrt(((p - q) ** 2).sum(-1))
    r = 1.0 / (d + 1e-8)
    w = r / r.sum(-1, keepdim=True)
    dy = dy0.double()
    pd = proj.double()
    a = torch.stack([(dy * torch.gather(pd, 2, il[..., j].unsqueeze(1).expand(-1, pd.shape[1], -1))).sum(1)
                     for j in range(3)], -1)                                    # (B, K*64, 3)
    v = torch.einsum("bmn,mc->bnc", dy, w0xyz.double())                        # (B, K*64, 3)
    loss = (a * w).sum() + (v * rel.reshape(b, -1, 3)).sum()
    gc, gs = torch.autograd.grad(loss, (c, s))
    return gc, gs


@pytest.mark.parametrize("b,k,nseed,ch", [(8, 256, 1024, 256), (1, 37, 1024, 256), (3, 13, 300, 64)])
def test_box_step_kernel_matches_float64_formula(b, k, nseed, ch):
    _, _, L = _mods()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(b * 1000 + k)
    m = 128
    seed_xyz = (torch.rand(b, nseed, 3, device=dev, generator=g) * torch.tensor([6.0, 5.0, 3.0], device=dev))
    center = torch.rand(b, k, 3, device=dev, generator=g) * torch.tensor([6.0, 5.0, 3.0], device=dev)
    size = torch.rand(b, k, 3, device=dev, generator=g) * 0.6 + 0.05
    heading = (torch.rand(b, k, device=dev, generator=g) - 0.5) * 6.0
    idx = torch.randint(0, nseed, (b, k * 64, 3), device=dev, generator=g, dtype=torch.int32)
    w0 = torch.randn(m, 3 + ch, device=dev, generator=g) * 0.1
    feats = torch.randn(b, ch, nseed, device=dev, generator=g)
    proj = torch.matmul(w0[:, 3:], feats).contiguous()
    dy0 = torch.randn(b, m, k * 64, device=dev, generator=g) * 1e-3
    unit = _unit(dev)
    grad = torch.empty(b, k, 6, device=dev)
    c1, s1 = center.clone(), size.clone()
    rate = 0.25
    with torch.cuda.device(dev):
        L.check(L.lib.votenet_iou_opt_box_step(
            b, k, nseed, m, unit.data_ptr(), seed_xyz.data_ptr(), idx.data_ptr(), proj.data_ptr(),
            w0.data_ptr(), w0.shape[1], dy0.data_ptr(), None, None, None, None, heading.data_ptr(), rate,
            c1.data_ptr(), s1.data_ptr(), grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "votenet_iou_opt_box_step")
    torch.cuda.synchronize()
    gc, gs = _formula_f64(unit, seed_xyz, idx, proj, w0[:, :3], dy0, center, size, heading)
    want = torch.cat([gc, gs], -1)
    scale = want.abs().amax(dim=(1, 2), keepdim=True)  # per-batch gradient scale
    err = ((grad.double() - want).abs() / scale).max().item()
    assert err < 1e-5, err
    torch.testing.assert_close(c1, center + rate * grad[..., :3], rtol=0, atol=1e-6)
    torch.testing.assert_close(s1, size + rate * grad[..., 3:], rtol=0, atol=1e-6)
    # deterministic: the same launch twice gives the same bits
    grad2 = torch.empty_like(grad)
    c2, s2 = center.clone(), size.clone()
    with torch.cuda.device(dev):
        L.check(L.lib.votenet_iou_opt_box_step(
            b, k, nseed, m, unit.data_ptr(), seed_xyz.data_ptr(), idx.data_ptr(), proj.data_ptr(),
            w0.data_ptr(), w0.shape[1], dy0.data_ptr(), None, None, None, None, heading.data_ptr(), rate,
            c2.data_ptr(), s2.data_ptr(), grad2.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "votenet_iou_opt_box_step")
    assert torch.equal(grad, grad2)


def _scene(tag, b=8, n=40000):
    V, O, _ = _mods()
    step = importlib.import_module("3dioumatch_amd.votenet.step")
    data = importlib.import_module("3dioumatch_amd.votenet.data")
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    det = step.build_detector(cfg, seed=0).cuda().eval()
    batch = data.make_batch(b, n, cfg, seed=3, device="cuda:0")
    with torch.no_grad():
        ep = det({"point_clouds": batch["point_clouds"]})
    return det, ep, cfg


def _agree(g_hip, g_ref):
    """per box: |g_hip - g_ref| <= 1e-3 |g_ref| (6-vectors); returns (fraction agreeing, count not)"""
    h = torch.cat(g_hip, -1).double()
    r = torch.cat(g_ref, -1).double()
    floor = 1e-6 * r.norm(dim=-1).max()
    ok = (h - r).norm(dim=-1) <= 1e-3 * r.norm(dim=-1) + floor
    return ok.float().mean().item(), int((~ok).sum().item())


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_engine_gradient_matches_autograd_at_the_same_boxes(tag):
    _, O, _ = _mods()
    det, ep, _ = _scene(tag)
    sem_cls = torch.argmax(ep["sem_cls_scores"], -1)
    center, size = ep["center"].detach(), ep["size"].detach()
    _, gc, gs = O._autograd_pass(det, ep, center, size, ep["heading"], sem_cls)
    run = O.HipBoxStep(det, ep)
    hc, hs = run.gradient(center, size)
    frac, bad = _agree((hc, hs), (gc, gs))
    print("%s: %d of %d boxes outside 1e-3" % (tag, bad, sem_cls.numel()))
    assert frac >= 0.995, (frac, bad)
    assert torch.cat([gc, gs], -1).abs().max() > 0


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_engine_trajectory_step_by_step(tag):
    _, O, _ = _mods()
    det, ep, cfg = _scene(tag)
    sem_cls = torch.argmax(ep["sem_cls_scores"], -1)
    heading = ep["heading"]
    center, size = ep["center"].detach(), ep["size"].detach()
    run = O.HipBoxStep(det, ep)
    _, gc, gs = O._autograd_pass(det, ep, center, size, heading, sem_cls)
    rate = 0.01 / torch.cat([gc, gs], -1).abs().median().item()
    opt_step = 10
    worst = 1.0
    for _ in range(opt_step + 1):
        hc, hs = run.gradient(center, size)  # the HIP update from the autograd trajectory's boxes
        frac, bad = _agree((hc, hs), (gc, gs))
        worst = min(worst, frac)
        assert frac >= 0.995, (frac, bad)
        center, size = center + rate * gc, size + rate * gs
        _, gc, gs = O._autograd_pass(det, ep, center, size, heading, sem_cls)
    assert (center - ep["center"]).abs().max() > 1e-3  # the boxes moved
    print("%s: worst step %.4f of the boxes within 1e-3" % (tag, worst))

    out = O.optimize_boxes(det, ep, rate, opt_step, engine="hip")
    b, k = sem_cls.shape
    ns = cfg.num_size_cluster
    assert out["center"].shape == (b, k, 3) and out["iou_scores"].shape == (b, k, cfg.num_class)
    assert out["size_residuals"].shape == (b, k, ns, 3)
    sr = out["size_residuals"]
    assert torch.equal(sr, sr[:, :, :1].expand(-1, -1, ns, -1))  # broadcast over the size clusters
    size_class = torch.argmax(ep["size_scores"], -1)
    half = (sr[:, :, 0] + det._mean_size[size_class]) / 2
    assert (half - ep["size"]).abs().max() > 0  # the final sizes, not the initial ones
    for key in ("heading", "size", "sem_cls_scores", "objectness_scores", "heading_residuals"):
        assert out[key] is ep[key]
    assert torch.isfinite(out["iou_scores"]).all() and torch.isfinite(out["center"]).all()


def test_engine_has_no_host_synchronisation():
    """one batch's refinement captured in a graph on one stream and replayed once == the eager run"""
    _, O, _ = _mods()
    det, ep, _ = _scene("scannet")
    rate, opt_step = 1e-3, 3
    eager = O.optimize_boxes(det, ep, rate, opt_step, engine="hip")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = O.optimize_boxes(det, ep, rate, opt_step, engine="hip")
    graph.replay()
    torch.cuda.synchronize()
    for key in ("center", "size_residuals", "iou_scores"):
        torch.testing.assert_close(captured[key], eager[key], rtol=0, atol=1e-6)
