"""GPU: the backward kernels that scatter-add through an index are repeatable -- the same inputs
give the same bits on every launch -- where many entries meet on one point (runs of the inverse
index that cross hundreds of lanes, same-address LDS adds from every wave), and they stay within
the fp32 bound of a float64 evaluation.  Then the whole train step: two runners from the same
state on the same batch agree bit for bit after two steps (bench.py --dump-outputs relies on it).

Kernels: group_inverse_kernel (the order of a point's entries), pregather_backward_kernel (runs
that cross lanes summed in lane order), three_interpolate_grad_lds_kernel (one LDS copy of the
rows per wave, copies summed in wave order).  Same-address LDS atomics issued by ONE wave
instruction are taken to be applied in a fixed lane order by the hardware; these tests check it.
"""
import importlib

import numpy as np
import pytest
import torch

from conftest import load_pkg

DEV = "cuda"
LAUNCHES = 8


def _repeat(fn):
    first = fn()
    torch.cuda.synchronize()
    for _ in range(LAUNCHES - 1):
        again = fn()
        assert torch.equal(first, again), "two launches on the same inputs gave different bits"
    return first


def _heavy_idx(b, n, m, ns, seed):
    """Cloud 0: every entry on point 0 (one run over all lanes); cloud 1: group j entirely on
    point j % 4 (runs of m / 4 * ns entries); the rest: ball-query style (first hit repeated)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32)
    idx[:, :, ns // 2:] = idx[:, :, :1]
    idx[0] = 0
    idx[1] = (torch.arange(m, dtype=torch.int32) % 4).view(m, 1)
    return idx.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,ns", [(2048, 1024, 32), (1024, 512, 16), (512, 256, 16)])
def test_group_inverse_is_repeatable(n, m, ns):
    load_pkg()
    ext = importlib.import_module("pointnet2._ext")
    idx = _heavy_idx(3, n, m, ns, seed=n + m)
    inv = _repeat(lambda: ext.group_inverse(idx, n))
    entries = inv.shape[1]
    chunk = entries // 1024
    packed = inv.cpu().numpy().view(np.uint32).reshape(3, chunk, 1024).transpose(0, 2, 1).reshape(3, entries)
    packed = packed[:, :m * ns]
    assert np.all(np.diff((packed >> 16).astype(np.int64), axis=1) >= 0)  # still sorted by point
    assert np.array_equal(np.sort(packed & 0xFFFF, axis=1),
                          np.broadcast_to(np.arange(m * ns, dtype=np.uint32), (3, m * ns)))


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,ns,c", [(2048, 1024, 32, 8), (1024, 512, 16, 8), (512, 256, 4, 4)])
def test_pregather_backward_is_repeatable_and_sums_runs_across_lanes(n, m, ns, c):
    load_pkg()
    ext = importlib.import_module("pointnet2._ext")
    K = importlib.import_module("pointnet2._mlp_ext")
    b = 3
    idx = _heavy_idx(b, n, m, ns, seed=7 * n + ns)
    inv = ext.group_inverse(idx, n)
    g = torch.Generator().manual_seed(m + c)
    y1 = torch.randn(b, c, m, ns, generator=g).to(DEV)
    dz1 = torch.randn(b, c, m, ns, generator=g).to(DEV)
    gamma = (torch.rand(c, generator=g) + 0.5).to(DEV)
    beta = torch.zeros(c, device=DEV)
    rmean, rvar = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    mean, invstd, scale, shift = K.bn_coefficients(y1, gamma, beta, rmean, rvar, 0.1, 1e-5, True)
    _, _, coef = K.bn_relu_backward_stats(y1, dz1, gamma, scale, shift, mean, invstd, True)
    fly = (y1, dz1, scale, shift, mean, invstd, coef)
    out = _repeat(lambda: K.pregather_backward(fly, inv, n)).double().cpu()
    scatter, groups = out[:, :, :n], -out[:, :, n:]  # (b, c, n), (b, c, m): sums of dy1 per group
    mass = groups.abs().sum(-1, keepdim=True)
    tol = 1e-5 * mass + 1e-4
    # cloud 0: everything on point 0; cloud 1: point p collects the groups j = p (mod 4)
    assert torch.all((scatter[0, :, :1] - groups[0].sum(-1, keepdim=True)).abs() <= tol[0])
    assert torch.all(scatter[0, :, 1:] == 0)
    want1 = torch.stack([groups[1, :, p::4].sum(-1) for p in range(4)], dim=-1)
    assert torch.all((scatter[1, :, :4] - want1).abs() <= tol[1])
    assert torch.all(scatter[1, :, 4:] == 0)
    # every cloud: the scatter conserves the total
    assert torch.all((scatter.sum(-1) - groups.sum(-1)).abs() <= tol[..., 0])


@pytest.mark.gpu
@pytest.mark.parametrize("b,c,m,n", [(2, 64, 512, 2048), (2, 256, 256, 1024), (1, 9, 1024, 4096)])
def test_three_interpolate_grad_is_repeatable(oracle, b, c, m, n):
    load_pkg()
    ext = importlib.import_module("pointnet2._ext")
    g = np.random.default_rng(b * c + m + n)
    idx = g.integers(0, m, (b, n, 3)).astype(np.int32)
    idx[0, : n // 2] = np.arange(3, dtype=np.int32)  # half the queries of a cloud on three points
    w = g.random((b, n, 3)).astype(np.float32)
    w = (w / w.sum(axis=2, keepdims=True)).astype(np.float32)
    go = g.standard_normal((b, c, n)).astype(np.float32)
    d_go, d_idx, d_w = (torch.from_numpy(a).to(DEV) for a in (go, idx, w))
    got = _repeat(lambda: ext.three_interpolate_grad(d_go, d_idx, d_w, m)).cpu().numpy()
    truth, mass = np.zeros((b, c, m)), np.zeros((b, c, m))
    for bi in range(b):
        for k in range(3):
            contrib = go[bi].astype(np.float64) * w[bi, :, k].astype(np.float64)
            np.add.at(truth[bi], (slice(None), idx[bi, :, k]), contrib)
            np.add.at(mass[bi], (slice(None), idx[bi, :, k]), np.abs(contrib))
    assert np.all(np.abs(got - truth) <= 1e-5 + 1e-6 * mass)
    np.testing.assert_allclose(got, oracle.three_interpolate_grad(go, idx, w, m), rtol=0,
                               atol=1e-5 + 1e-6 * mass.max())


@pytest.mark.gpu
def test_train_step_is_repeatable():
    """Two runners from the same initial state, two steps on the same batches (HIP graphs, the
    index chain prefetched as bench.py runs it): loss, every end_points tensor and the parameters
    agree bit for bit."""
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    data = importlib.import_module("3dioumatch_amd.votenet.data")
    cfg = V.scannet_config()
    dev = torch.device(DEV, 0)
    batches = [data.make_batch(2, 20000, cfg, seed=s, num_objects=5, device=dev) for s in (44, 45)]

    def run():
        runner = V.SupervisedStep(cfg, dev, world_size=1, num_proposal=64, seed=3, graphs=True)
        torch.manual_seed(9)
        views = [dict(bt) for bt in batches]
        runner.prefetch_geometry(views[0])
        out = []
        for i in range(2):
            if i + 1 < len(views):
                runner.prefetch_geometry(views[i + 1])
            loss, ep = runner(views[i])
            out.append({k: v.detach().clone() for k, v in ep.items() if torch.is_tensor(v)})
            out[-1]["_loss"] = loss.detach().clone()
        torch.cuda.synchronize()
        out.append({"_params": runner.flat_params.detach().clone()})
        assert runner.graphs
        return out

    first, second = run(), run()
    for step, (a, b) in enumerate(zip(first, second)):
        differ = [k for k in a if not torch.equal(a[k], b[k])]
        assert not differ, (step, differ)
