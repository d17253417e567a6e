"""GPU tests of the fused BatchNorm(+ReLU)(+max-pool) kernels behind SharedMLP against plain
torch ops on the same device (fp32 reference of the same op): forward values, running
statistics, and gradients w.r.t. input, gamma, beta -- training and eval mode, vector and
ragged shapes.  Tolerance 1e-4 (relative to the tensor scale)."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _mods():
    load_pkg()
    return importlib.import_module("pointnet2.pytorch_utils")


def close(a, b, tol=1e-4):
    a, b = a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy()
    scale = max(1.0, float(np.abs(b).max()))
    assert np.abs(a - b).max() <= tol * scale, float(np.abs(a - b).max())


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _f64_twin(ref):
    """nn.Sequential of the same modules in float64: the TRUTH both fp32 paths are measured against."""
    import copy
    twin = copy.deepcopy(ref).double()
    twin.train(ref.training)
    return twin


def _grad_bound(got, ref32, truth, floor=2e-3):
    """tests/test_train_step.py:84-131's rule for a gradient that is a sum with ReLU / arg-max gates
    within rounding of a tie: ANY fp32 evaluation sits rel(ref32, truth) away from the float64
    value (its own round-off and its own flipped gates), so the kernel's result may be three times
    that + `floor` away from the truth -- tight where the sum is well conditioned and never looser
    than what fp32 torch itself resolves.  (Before round 6: a blanket rel < 3e-2 against ref32.)"""
    e_ref, e_got = _rel(ref32, truth), _rel(got, truth)
    assert e_got <= floor + 3 * e_ref, (e_got, e_ref)
    return e_got, e_ref


@pytest.mark.parametrize("shape", [(2, 7, 33, 5), (2, 16, 40, 16), (3, 64, 100, 64),
                                   (2, 8, 50, 32), (2, 5, 1000, 1), (1, 3, 7, 8), (4, 128, 64, 4)])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("pool", [False, True])
def test_bn_relu_pool_vs_torch(shape, training, pool):
    P = _mods()
    g = torch.Generator().manual_seed(sum(shape))
    b, c, m, ns = shape
    y0 = (torch.randn(shape, generator=g) * 2 + 0.5).to(DEV)
    gamma0 = (torch.rand(c, generator=g) + 0.5).to(DEV)
    gamma0[0] = -0.7  # negative scale: max and relu must not be commuted blindly
    beta0 = (torch.randn(c, generator=g) * 0.3).to(DEV)
    rm0 = (torch.randn(c, generator=g) * 0.1).to(DEV)
    rv0 = (torch.rand(c, generator=g) + 0.5).to(DEV)
    w = torch.randn((b, c, m) if pool else shape, generator=g).to(DEV)

    def run(fused):
        y = y0.clone().requires_grad_(True)
        gamma = gamma0.clone().requires_grad_(True)
        beta = beta0.clone().requires_grad_(True)
        rm, rv = rm0.clone(), rv0.clone()
        if fused:
            op = P._BNReLUMaxPool if pool else P._BNReLU
            out = op.apply(y, gamma, beta, rm, rv, 0.1, 1e-5, training)
        else:
            z = F.relu(F.batch_norm(y, rm, rv, gamma, beta, training, 0.1, 1e-5))
            out = torch.max(z, dim=3)[0] if pool else z
        (out * w).sum().backward()
        return out, y.grad, gamma.grad, beta.grad, rm, rv

    got, want = run(True), run(False)
    names = ["out", "dy", "dgamma", "dbeta", "running_mean", "running_var"]
    for n, a, bb in zip(names, got, want):
        tol = 1e-4 if n in ("out", "running_mean", "running_var") else 3e-4
        close(a, bb, tol)


def test_shared_mlp_fused_matches_sequential():
    """SharedMLP on the GPU (fused path) == the same module evaluated layer by layer with torch
    ops (its nn.Sequential definition), forward + backward, incl. forward_pooled."""
    P = _mods()
    torch.manual_seed(0)
    mlp = P.SharedMLP([6, 16, 16, 32], bn=True).to(DEV).train()
    ref = P.SharedMLP([6, 16, 16, 32], bn=True).to(DEV).train()
    ref.load_state_dict(mlp.state_dict())
    x1 = torch.randn(3, 6, 50, 16, device=DEV, requires_grad=True)
    x2 = x1.detach().clone().requires_grad_(True)
    out = mlp.forward_pooled(x1)
    z = torch.nn.Sequential.forward(ref, x2)
    want = torch.max(z, dim=3)[0]
    close(out, want)
    wgt = torch.randn_like(want)
    (out * wgt).sum().backward()
    (want * wgt).sum().backward()
    close(x1.grad, x2.grad, 3e-4)
    for (n1, p1), (n2, p2) in zip(mlp.named_parameters(), ref.named_parameters()):
        close(p1.grad, p2.grad, 3e-4)
    for (n1, b1), (n2, b2) in zip(mlp.named_buffers(), ref.named_buffers()):
        close(b1.float(), b2.float())
    mlp.eval(); ref.eval()
    with torch.no_grad():
        close(mlp(x1), torch.nn.Sequential.forward(ref, x2))


@pytest.mark.parametrize("b,m,k,r", [(2, 64, 4, 640), (1, 128, 64, 1000), (2, 256, 131, 512),
                                     (3, 259, 128, 96), (1, 3, 7, 33), (2, 131, 259, 1024),
                                     (1, 512, 256, 64), (2, 32, 512, 200), (2, 64, 64, 3001),
                                     (1, 100, 100, 2050), (2, 70, 160, 1537), (1, 65, 300, 777),
                                     # column counts the pipelined kernels take (r % 256 == 0),
                                     # every tile shape, K below / at / across the 16-deep chunk
                                     (1, 64, 4, 1024), (2, 64, 64, 512), (1, 128, 64, 256),
                                     (2, 40, 16, 768), (1, 96, 17, 512), (2, 300, 128, 256)])
@pytest.mark.parametrize("small", [True, False], ids=["small-tile", "big-tile"])
def test_mfma_gemm_primitives_vs_torch(b, m, k, r, small, monkeypatch):
    """forward / dgrad / wgrad of the 1x1 convolution on the matrix cores, every operand mode,
    ragged M, K, R -- against torch matmul of explicitly materialised operands (fp32); both the
    64x64 latency-oriented kernel and the large-tile kernels."""
    monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "1000000000" if small else "0")
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(b * 1000 + m + k + r)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = torch.randn(b, k, r, generator=g).to(DEV)
    scale_k = (torch.rand(k, generator=g) + 0.5).to(DEV)
    shift_k = (torch.randn(k, generator=g) * 0.3).to(DEV)
    # forward, direct and with the BN+ReLU prologue
    close(K.gemm_forward(w, x), torch.matmul(w, x), 2e-5)
    xz = torch.relu(x * scale_k[None, :, None] + shift_k[None, :, None])
    close(K.gemm_forward(w, x, (scale_k, shift_k)), torch.matmul(w, xz), 2e-5)
    # the on-the-fly dy operand
    y = torch.randn(b, m, r, generator=g).to(DEV)
    dz = torch.randn(b, m, r, generator=g).to(DEV)
    sc = (torch.rand(m, generator=g) + 0.5).to(DEV)
    sh = (torch.randn(m, generator=g) * 0.3).to(DEV)
    mu = (torch.randn(m, generator=g) * 0.2).to(DEV)
    istd = (torch.rand(m, generator=g) + 0.5).to(DEV)
    coef = torch.stack([torch.rand(m, generator=g) + 0.5, torch.randn(m, generator=g) * 0.1,
                        torch.randn(m, generator=g) * 0.1], dim=1).contiguous().to(DEV)
    bc = lambda v: v[None, :, None]  # noqa: E731
    mask = (y * bc(sc) + bc(sh) > 0).float()
    dy = bc(coef[:, 0]) * (dz * mask - bc(coef[:, 1]) - (y - bc(mu)) * bc(istd) * bc(coef[:, 2]))
    fly = (y, dz, sc, sh, mu, istd, coef)
    want_dx = torch.matmul(w.t(), dy)
    close(K.gemm_dgrad(w, dy=dy.contiguous()), want_dx, 3e-5)
    close(K.gemm_dgrad(w, fly=fly), want_dx, 3e-5)
    want_dw_direct = torch.einsum("bmr,bkr->mk", dy, x)
    want_dw_bn = torch.einsum("bmr,bkr->mk", dy, xz)
    tol = 1e-4
    close(K.gemm_wgrad(m, k, x, None, dy=dy.contiguous()), want_dw_direct, tol)
    close(K.gemm_wgrad(m, k, x, (scale_k, shift_k), dy=dy.contiguous()), want_dw_bn, tol)
    close(K.gemm_wgrad(m, k, x, None, fly=fly), want_dw_direct, tol)
    close(K.gemm_wgrad(m, k, x, (scale_k, shift_k), fly=fly), want_dw_bn, tol)


@pytest.mark.parametrize("b,m,k,r", [(2, 64, 4, 1024), (3, 128, 64, 512), (2, 256, 128, 768),
                                     (1, 96, 131, 16640), (8, 128, 128, 4096)])
@pytest.mark.parametrize("offset", [0.0, 40.0])
def test_forward_gemm_leaves_batchnorm_statistics(b, m, k, r, offset):
    """Training-mode layer with the batch statistics reduced in the GEMM epilogue
    (mlp_gemm_forward with pairs + mlp_bn_finalize_pairs) == the GEMM followed by the statistics pass
    over y (and == torch): same y, same mean / invstd / scale / shift, same running statistics --
    also when the channel means are 40 standard deviations away from zero (shifted sums)."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(b + m + k + r)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = (torch.randn(b, k, r, generator=g) + offset).to(DEV)
    gamma = (torch.rand(m, generator=g) + 0.5).to(DEV)
    beta = torch.randn(m, generator=g).to(DEV)
    coeff = None
    if k > 4:
        coeff = ((torch.rand(k, generator=g) + 0.5).to(DEV), (torch.randn(k, generator=g) * 0.3).to(DEV))
    rm1, rv1 = torch.zeros(m, device=DEV), torch.ones(m, device=DEV)
    rm2, rv2 = torch.zeros(m, device=DEV), torch.ones(m, device=DEV)
    y1, mean1, inv1, sc1, sh1 = K.gemm_forward_bn(w, x, coeff, gamma, beta, rm1, rv1, 0.1, 1e-5)
    y2 = K.gemm_forward(w, x, coeff)
    mean2, inv2, sc2, sh2 = K.bn_coefficients(y2, gamma, beta, rm2, rv2, 0.1, 1e-5, True)
    assert torch.equal(y1, y2)
    ref = y2.double()
    want_mean = ref.mean(dim=(0, 2))
    want_var = ref.var(dim=(0, 2), unbiased=False)
    scale = float(want_var.sqrt().max())
    assert float((mean1.double() - want_mean).abs().max()) <= 2e-6 * max(1.0, float(want_mean.abs().max()), scale)
    assert float((inv1.double() * torch.sqrt(want_var + 1e-5) - 1).abs().max()) <= 2e-5
    close(mean1, mean2, 1e-6); close(inv1, inv2, 2e-5); close(sc1, sc2, 2e-5); close(sh1, sh2, 2e-5)
    close(rm1, rm2, 1e-6); close(rv1, rv2, 2e-5)


@pytest.mark.parametrize("b,m,k,groups,ns", [(2, 128, 64, 50, 64), (1, 256, 131, 33, 32),
                                             (2, 70, 259, 17, 16), (1, 64, 20, 40, 6),
                                             (2, 33, 7, 9, 3)])
def test_pooled_operand_mode_vs_materialised(b, m, k, groups, ns):
    """dgrad / wgrad of a pooled last layer with dy rebuilt inside the operand loads from
    (y, dpooled, argmax) == the same GEMMs on the dy tensor written out by the BN/pool backward."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(m * 7 + k + groups + ns)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = torch.randn(b, k, groups, ns, generator=g).to(DEV)
    y = torch.randn(b, m, groups, ns, generator=g).to(DEV)
    gamma = (torch.rand(m, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(m, generator=g) * 0.3).to(DEV)
    rm, rv = torch.zeros(m, device=DEV), torch.ones(m, device=DEV)
    mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, rm, rv, 0.1, 1e-5, True)
    pooled, argmax, ymax = K.bn_relu_pool(y, scale, shift)
    dpooled = torch.randn(b, m, groups, generator=g).to(DEV)
    dy, dgamma, dbeta = K.bn_relu_pool_backward(y, dpooled, argmax, ymax, gamma, scale, shift, mean,
                                                invstd, True)
    dgamma2, dbeta2, coef = K.bn_relu_pool_backward_stats(y, dpooled, argmax, ymax, gamma, scale,
                                                          shift, mean, invstd, True)
    close(dgamma2, dgamma, 1e-6); close(dbeta2, dbeta, 1e-6)
    op = (y, dpooled, argmax, scale, shift, mean, invstd, coef)
    close(K.gemm_dgrad(w, pooled=op), K.gemm_dgrad(w, dy=dy), 1e-5)
    scale_k = (torch.rand(k, generator=g) + 0.5).to(DEV)
    shift_k = (torch.randn(k, generator=g) * 0.3).to(DEV)
    close(K.gemm_wgrad(m, k, x, None, pooled=op), K.gemm_wgrad(m, k, x, None, dy=dy), 1e-5)
    close(K.gemm_wgrad(m, k, x, (scale_k, shift_k), pooled=op),
          K.gemm_wgrad(m, k, x, (scale_k, shift_k), dy=dy), 1e-5)


@pytest.mark.parametrize("b,m,k,groups,ns,pooled", [
    (2, 64, 64, 40, 64, False), (2, 128, 64, 36, 64, True), (3, 128, 64, 301, 64, True), (3, 128, 128, 25, 32, False),
    (2, 256, 128, 33, 32, True), (2, 128, 131, 40, 32, False), (5, 128, 259, 26, 16, False),
    (8, 128, 128, 512, 16, False), (1, 256, 128, 2048, 16, True), (2, 128, 128, 64, 64, True),
    (3, 128, 128, 256, 16, True)])
def test_fused_backward_vs_two_gemms(b, m, k, groups, ns, pooled):
    """dgrad + wgrad of a layer from ONE pass over its activations (mlp_gemm_backward_fused) ==
    the two separate on-the-fly GEMMs, for every layer shape of the network: gradient operand from
    (y, dz) or from the pooled tensors, input operand direct (grouped input, 3 coordinate rows in
    front) or relu(bn(.)); several chunks per workgroup and ragged chunk counts."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(m * 7 + k + groups + ns)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = torch.randn(b, k, groups, ns, generator=g).to(DEV)
    y = torch.randn(b, m, groups, ns, generator=g).to(DEV)
    gamma = (torch.rand(m, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(m, generator=g) * 0.3).to(DEV)
    rm, rv = torch.zeros(m, device=DEV), torch.ones(m, device=DEV)
    mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, rm, rv, 0.1, 1e-5, True)
    if pooled:
        _, argmax, ymax = K.bn_relu_pool(y, scale, shift)
        dpooled = torch.randn(b, m, groups, generator=g).to(DEV)
        _, _, coef = K.bn_relu_pool_backward_stats(y, dpooled, argmax, ymax, gamma, scale, shift,
                                                   mean, invstd, True)
        kw = dict(pooled=(y, dpooled, argmax, scale, shift, mean, invstd, coef))
    else:
        dz = torch.randn(b, m, groups, ns, generator=g).to(DEV)
        _, _, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, True)
        kw = dict(fly=(y, dz, scale, shift, mean, invstd, coef))
    xcoeff = xstats = None
    if k % 32 == 0:  # not a grouped network input: the previous layer's raw output
        xgamma = (torch.rand(k, generator=g) + 0.5).to(DEV)
        xbeta = (torch.randn(k, generator=g) * 0.3).to(DEV)
        xmean, xinv, xscale, xshift = K.bn_coefficients(x, xgamma, xbeta, torch.zeros(k, device=DEV),
                                                        torch.ones(k, device=DEV), 0.1, 1e-5, True)
        xcoeff, xstats = (xscale, xshift), (xmean, xinv, xgamma, True)
    both = K.gemm_backward_fused(w, x, xcoeff, xstats=xstats, **kw)
    assert both is not None, "shape not routed to the fused kernel"
    dx, dw, below = both
    want_dx = K.gemm_dgrad(w, **kw).view_as(x)
    want_dw = K.gemm_wgrad(m, k, x, xcoeff, **kw)
    close(dx, want_dx, 1e-5)
    close(dw, want_dw, 2e-5)
    if (m, k) == (128, 259):  # the form for a first layer whose input needs no gradient
        none, dw_only, _ = K.gemm_backward_fused(w, x, xcoeff, xstats=xstats, need_dx=False, **kw)
        assert none is None
        close(dw_only, want_dw, 2e-5)
    # the first set-abstraction level's layers, and the (128,128) layers on the bf16-split kernel
    assert (below is not None) == (k == 64 or (m, k) == (128, 128))
    if below is not None:  # the layer below's BatchNorm-backward sums == its stats pass over (x, dx)
        dgamma, dbeta, coef = K.bn_relu_backward_stats(x, want_dx.contiguous(), xgamma, xscale, xshift,
                                                       xmean, xinv, True)
        close(below[0], dgamma, 2e-5); close(below[1], dbeta, 2e-5); close(below[2], coef, 2e-5)


def test_fused_backward_declines_other_shapes():
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    z = lambda *s: torch.zeros(*s, device=DEV)
    fly = lambda m, *s: (z(2, m, *s), z(2, m, *s), z(m), z(m), z(m), z(m), z(3, m))
    assert K.gemm_backward_fused(z(96, 64), z(2, 64, 64, 64), (z(64), z(64)), fly=fly(96, 64, 64)) is None
    assert K.gemm_backward_fused(z(128, 128), z(2, 128, 10, 31), (z(128), z(128)), fly=fly(128, 10, 31)) is None
    assert K.gemm_backward_fused(z(128, 128), z(2, 128, 4, 32), (z(128), z(128)), fly=fly(128, 4, 32)) is None


@pytest.mark.parametrize("widths,shape", [([4, 64, 64, 128], (2, 4, 64, 64)),
                                          ([131, 128, 128, 256], (2, 131, 50, 32)),
                                          ([131, 128, 128, 256], (4, 131, 256, 32)),
                                          ([259, 128, 128, 256], (3, 259, 512, 16)),
                                          ([259, 128, 128], (3, 259, 20, 16)),
                                          ([20, 8], (2, 20, 300, 1))])
@pytest.mark.parametrize("training", [True, False])
def test_fused_chain_vs_sequential(widths, shape, training, monkeypatch):
    """The one-node MFMA chain (SharedMLP on the GPU) == nn.Sequential of the same modules:
    pooled and unpooled forward, input / weight / BN gradients, running statistics.  The two larger
    128 -> 128 -> 256 cases run SA2's form: the last layer's raw output is never stored, its backward
    comes from the Gram matrix of its input (csrc/mlp_pool_gram256.hip)."""
    P = _mods()
    K = importlib.import_module("pointnet2._mlp_ext")
    monkeypatch.setenv("MLP_POOL_GRAM256_MIN_CHUNKS", "64")  # (the product: from 4096 chunks on)
    gram_calls = []
    real_gram = K.pool_gram_backward
    monkeypatch.setattr(K, "pool_gram_backward", lambda *a, **k: (gram_calls.append(1), real_gram(*a, **k))[1])
    torch.manual_seed(1)
    mlp = P.SharedMLP(list(widths), bn=True).to(DEV)
    ref = P.SharedMLP(list(widths), bn=True).to(DEV)
    ref.load_state_dict(mlp.state_dict())
    mlp.train(training); ref.train(training)
    for pool in (True, False):
        x1 = torch.randn(shape, device=DEV, requires_grad=True)
        x2 = x1.detach().clone().requires_grad_(True)
        out = mlp.forward_pooled(x1) if pool else mlp(x1)
        z = torch.nn.Sequential.forward(ref, x2)
        want = torch.max(z, dim=3)[0] if pool else z
        close(out, want, 2e-4)
        wgt = torch.randn_like(want)
        mlp.zero_grad(); ref.zero_grad()
        (out * wgt).sum().backward()
        (want * wgt).sum().backward()
        # The two forwards differ in the last ulp (different summation order), so a pre-activation
        # within rounding of 0 can flip its ReLU mask, and a max over nsample can pick another
        # near-tied sample: either moves the gradient of ONE column.  Compare robustly: almost
        # every element agrees tightly, and the dense sums agree in relative L2.
        d = (x1.grad - x2.grad).abs()
        assert float((d > 5e-4 * max(1.0, float(x2.grad.abs().max()))).float().mean()) < 2e-3
        # weight / BatchNorm gradients: against the float64 evaluation of the same modules
        ref64 = _f64_twin(ref)  # (training: batch statistics; eval: the running ones, unchanged)
        ref64.zero_grad()
        x3 = x1.detach().double().requires_grad_(True)
        z64 = torch.nn.Sequential.forward(ref64, x3)
        want64 = torch.max(z64, dim=3)[0] if pool else z64
        (want64 * wgt.double()).sum().backward()
        worst = 0.0
        for (n1, p1), (n2, p2), (n3, p3) in zip(mlp.named_parameters(), ref.named_parameters(),
                                                ref64.named_parameters()):
            e_got, e_ref = _grad_bound(p1.grad, p2.grad, p3.grad)
            worst = max(worst, e_got / (2e-3 + 3 * e_ref))
        print("chain vs float64: worst gradient at %.2f of its bound" % worst)
        for (n1, b1), (n2, b2) in zip(mlp.named_buffers(), ref.named_buffers()):
            close(b1.float(), b2.float(), 2e-4)
    if training and widths[-1] == 256 and shape[2] * shape[3] >= 8192:
        assert len(gram_calls) == 1, "the pooled 128 -> 256 layer did not take the Gram path"


@pytest.mark.parametrize("cin,mid,cout,shape", [(256, 256, 259, (2, 1024)), (128, 128, 79, (3, 256)),
                                                (20, 12, 7, (2, 33))])
@pytest.mark.parametrize("training", [True, False])
def test_fused_head_chain_vs_torch(cin, mid, cout, shape, training):
    """conv1d-BN-ReLU x2 + conv1d of the vote / proposal / IoU heads on the MFMA + BN kernels ==
    the torch modules: output, every gradient, running statistics (bias folded correctly)."""
    load_pkg()
    fh = importlib.import_module("3dioumatch_amd.votenet.fused_head")
    nn = torch.nn
    torch.manual_seed(cin + cout)
    mods = [nn.Conv1d(cin, mid, 1), nn.BatchNorm1d(mid), nn.Conv1d(mid, mid, 1), nn.BatchNorm1d(mid),
            nn.Conv1d(mid, cout, 1)]
    for m in mods:
        if isinstance(m, nn.BatchNorm1d):
            m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.3)
            m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
        else:
            m.bias.data.normal_(0, 0.5)
    import copy
    ref = [copy.deepcopy(m).to(DEV) for m in mods]
    mods = [m.to(DEV) for m in mods]
    for m in mods + ref:
        m.train(training)
    b, r = shape
    x1 = torch.randn(b, cin, r, device=DEV, requires_grad=True)
    x2 = x1.detach().clone().requires_grad_(True)
    out = fh.head_chain(x1, *mods)
    os.environ["VOTENET_FUSED_HEADS"] = "0"
    try:
        want = fh.head_chain(x2, *ref)
    finally:
        os.environ.pop("VOTENET_FUSED_HEADS")
    close(out, want, 2e-4)
    gout = torch.randn_like(want)
    out.backward(gout)
    want.backward(gout)
    close(x1.grad, x2.grad, 5e-4)
    for m, q in zip(mods, ref):
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), q.named_parameters()):
            if training and n1 == "bias" and isinstance(m, torch.nn.Conv1d) and m is not mods[4]:
                assert float(p1.grad.abs().max()) == 0.0  # cancels in front of a batch-stat BN
                assert float(p2.grad.abs().max()) < 1e-3  # ... where torch accumulates noise
                continue
            close(p1.grad, p2.grad, 5e-4)
        for (n1, b1), (n2, b2) in zip(m.named_buffers(), q.named_buffers()):
            close(b1.float(), b2.float(), 1e-5)


@pytest.mark.parametrize("n,world,teacher", [(1000003, 1, False), (4096, 2, True), (5, 1, True)])
def test_flat_adam_step_matches_torch(n, world, teacher):
    """votenet_adam_step (Adam on one flat buffer, optional EMA teacher, gradient pre-scaled by
    1/world) == torch.optim.Adam + lerp_ over several steps, lr changed in between."""
    load_pkg()
    L = importlib.import_module("3dioumatch_amd._lib")
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g).to(DEV)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=2e-3)
    p = p0.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros((), device=DEV)
    lr = torch.tensor(2e-3, device=DEV)
    scratch = torch.zeros(2, device=DEV)
    ema = p0.clone() if teacher else None
    ema_ref = p0.clone()
    w = torch.zeros((), device=DEV)
    for it in range(4):
        grad = (torch.randn(n, generator=g) * (10.0 ** (it - 2))).to(DEV)
        if it == 2:
            lr.fill_(5e-4)
            opt.param_groups[0]["lr"] = 5e-4
        w.fill_(1.0 - min(1 - 1 / (it + 1), 0.999))
        ref.grad = grad / world
        opt.step()
        ema_ref.lerp_(ref.data, w)
        L.check(L.lib.votenet_adam_step(n, p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                                        step.data_ptr(), lr.data_ptr(), 0.9, 0.999, 1e-8, 0.0, 1.0 / world,
                                        ema.data_ptr() if teacher else None, w.data_ptr() if teacher else None,
                                        scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), "adam")
    assert float(step) == 4.0
    close(grad, ref.grad, 1e-7)  # the mean is left where the sum was
    close(p, ref.data, 2e-6)
    close(m, opt.state[ref]["exp_avg"], 2e-6)
    close(v, opt.state[ref]["exp_avg_sq"], 2e-6)
    if teacher:
        close(ema, ema_ref, 2e-6)


@pytest.mark.parametrize("shape", [(8, 256, 1024), (2, 7, 100), (1, 3, 1)])
def test_unit_length_features_vs_torch(shape):
    """votenet_channel_normalize[_grad] == features.div(torch.norm(features, p=2, dim=1).unsqueeze(1))
    and its autograd backward (models/votenet_iou_branch.py:103-104)."""
    load_pkg()
    D = importlib.import_module("3dioumatch_amd.votenet.detector")
    g = torch.Generator().manual_seed(sum(shape))
    x1 = (torch.randn(shape, generator=g) * 3).to(DEV).requires_grad_(True)
    x2 = x1.detach().clone().requires_grad_(True)
    y1 = D.unit_length_features(x1)
    y2 = x2.div(torch.norm(x2, p=2, dim=1).unsqueeze(1))
    close(y1, y2, 1e-6)
    wgt = torch.randn(shape, generator=g).to(DEV)
    (y1 * wgt).sum().backward()
    (y2 * wgt).sum().backward()
    close(x1.grad, x2.grad, 2e-6)


@pytest.mark.parametrize("b,m,k,groups,ns", [(5, 128, 64, 64, 64), (2, 256, 128, 512, 32), (1, 128, 128, 512, 64),
                                             (3, 256, 128, 128, 64), (5, 128, 128, 128, 32), (2, 256, 128, 1024, 16),
                                             (3, 128, 128, 512, 16)])
def test_pool_from_gemm_epilogue_extrema(b, m, k, groups, ns):
    """max over nsample of relu(bn(y)) from the per-group winner of the raw GEMM output
    (mlp_gemm_forward_stats_pool + mlp_bn_pool_from_extrema) == bn_relu_pool on y: pooled values
    and winning pre-activations identical, arg-max identical wherever the winner is not rectified
    to zero (there the gradient is zero whichever sample is named); channels with a negative
    BatchNorm scale take the minimum.  Groups with repeated samples (ball-query padding) keep the
    FIRST occurrence."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(m + k + groups + ns)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = torch.randn(b, k, groups, ns, generator=g)
    x[:, :, :, ns // 2:] = x[:, :, :, :1]  # padding: the first sample repeated
    x = x.to(DEV)
    xs, xh = (torch.rand(k, generator=g) + 0.5).to(DEV), (torch.randn(k, generator=g) * 0.3).to(DEV)
    gamma = (torch.rand(m, generator=g) + 0.5)
    gamma[::3] *= -1.0  # negative scales: the winner is the group's minimum
    gamma = gamma.to(DEV)
    beta = (torch.randn(m, generator=g) * 0.3).to(DEV)
    rm, rv = torch.zeros(m, device=DEV), torch.ones(m, device=DEV)
    y, mean, invstd, scale, shift, ext = K.gemm_forward_bn(w, x, (xs, xh), gamma, beta, rm, rv, 0.1, 1e-5,
                                                           pool=True)
    assert ext is not None, "shape not routed to the pooled epilogue"
    pooled, argmax, ymax = K.pool_from_extrema(ext, scale, shift)
    want_p, want_a, want_y = K.bn_relu_pool(y, scale, shift)
    assert torch.equal(pooled, want_p)
    live = want_p > 0
    assert torch.equal(argmax[live], want_a[live])
    assert torch.equal(ymax[live], want_y[live])
    # the named sample always holds the named value
    picked = torch.gather(y, 3, argmax.long().unsqueeze(3)).squeeze(3)
    assert torch.equal(picked, ymax)


@pytest.mark.parametrize("b,groups,ns,training", [(8, 256, 64, True), (2, 33, 4, True), (3, 100, 8, False)])
def test_first_layer_weight_gradient_from_moments(b, groups, ns, training):
    """mlp_wgrad_first4 (4 -> 64 first layer: gated sums over dz and x, the rest from the second
    moments of x; the layer's output is never read) == the general on-the-fly wgrad over (y, dz).
    (Against the float64 autograd, on inputs no kernel prepares: tests/test_sa1_train_gpu.py.)"""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(groups + ns)
    w = (torch.randn(64, 4, generator=g) * 0.5).to(DEV)
    x = (torch.randn(b, 4, groups, ns, generator=g) * 2 + 0.7).to(DEV)
    gamma = (torch.rand(64, generator=g) + 0.5)
    gamma[::5] *= -1
    gamma = gamma.to(DEV)
    beta = (torch.randn(64, generator=g) * 0.3).to(DEV)
    rm, rv = (torch.randn(64, generator=g) * 0.1).to(DEV), (torch.rand(64, generator=g) + 0.5).to(DEV)
    y = K.gemm_forward(w, x, None)
    mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, rm, rv, 0.1, 1e-5, training)
    dz = torch.randn(b, 64, groups, ns, generator=g).to(DEV)
    _, _, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, training)
    fly = (y, dz, scale, shift, mean, invstd, coef)
    got = K.wgrad_first4(w, x, fly)
    assert got is not None
    want = K.gemm_wgrad(64, 4, x, None, fly=fly)
    close(got, want, 3e-5)


@pytest.mark.parametrize("pool", [True, False])
def test_virtual_first_layer_chain_vs_sequential(pool, monkeypatch):
    """SA1's chain 4 -> 64 -> 64 -> 128 with the first layer VIRTUAL (its output never stored:
    BatchNorm statistics from the second moments of the input, its rows recomputed inside the
    second layer's forward and backward kernels, its weight gradient from gated sums + moments)
    == the same chain with the layer materialised, and == nn.Sequential: outputs, every parameter
    gradient, running statistics."""
    P = _mods()
    K = importlib.import_module("pointnet2._mlp_ext")
    torch.manual_seed(3)
    widths, shape = [4, 64, 64, 128], (8, 4, 256, 64)
    mlp = P.SharedMLP(list(widths), bn=True).to(DEV)
    for layer in mlp:
        bn = next(layer.bn.children())
        bn.weight.data.uniform_(0.5, 1.5)
        bn.weight.data[::7] *= -1
        bn.bias.data.normal_(0, 0.3)
    twin = P.SharedMLP(list(widths), bn=True).to(DEV)
    twin.load_state_dict(mlp.state_dict())
    ref = P.SharedMLP(list(widths), bn=True).to(DEV)
    ref.load_state_dict(mlp.state_dict())
    x = (torch.randn(shape, device=DEV) * 1.5 + 0.4)
    assert K.lin4_supported(mlp[0].conv.weight.reshape(64, 4), mlp[1].conv.weight.reshape(64, 64), x)
    calls = []
    real = K.first4_moments
    monkeypatch.setattr(K, "first4_moments", lambda t: (calls.append(1), real(t))[1])
    gram_calls = []
    real_gram = K.pool_gram_backward
    monkeypatch.setattr(K, "pool_gram_backward", lambda *a, **k: (gram_calls.append(1), real_gram(*a, **k))[1])
    out = mlp.forward_pooled(x) if pool else mlp(x)
    assert calls, "the first layer was materialised"
    monkeypatch.setenv("MLP_FIRST4_VIRTUAL", "0")
    out2 = twin.forward_pooled(x) if pool else twin(x)
    ref64 = _f64_twin(ref)  # (before the forward pass moves the running statistics)
    z = torch.nn.Sequential.forward(ref, x)
    want = torch.max(z, dim=3)[0] if pool else z
    close(out, out2, 1e-5)
    close(out, want, 2e-4)
    wgt = torch.randn_like(want)
    (out * wgt).sum().backward()
    # (pooled: layers 2 + 3 chained, the last raw output not stored, its backward from the Gram matrix)
    assert len(gram_calls) == (1 if pool else 0), "SA1's pooled last layer did not take the Gram path"
    (out2 * wgt).sum().backward()
    (want * wgt).sum().backward()
    z64 = torch.nn.Sequential.forward(ref64, x.double())
    ((torch.max(z64, dim=3)[0] if pool else z64) * wgt.double()).sum().backward()
    for (n1, p1), (n2, p2), (n3, p3), (n4, p4) in zip(mlp.named_parameters(), twin.named_parameters(),
                                                      ref.named_parameters(), ref64.named_parameters()):
        rel = float((p1.grad - p2.grad).norm() / (p2.grad.norm() + 1e-12))
        # virtual (+ layers 2 and 3 chained in registers, csrc/mlp_chain.hip) vs materialised,
        # layer by layer: other forward kernels, so ReLU masks within rounding of 0 may differ
        assert rel < 6e-3, (n1, rel)
        # vs torch: both fp32 results against the float64 evaluation (_grad_bound)
        _grad_bound(p1.grad, p3.grad, p4.grad)
    for (n1, b1), (n2, b2) in zip(mlp.named_buffers(), ref.named_buffers()):
        close(b1.float(), b2.float(), 2e-4)


@pytest.mark.parametrize("b,m,ns", [(8, 256, 64), (4, 512, 32), (2, 1024, 16), (8, 2048, 64)])
def test_chained_forward_vs_layerwise(b, m, ns):
    """csrc/mlp_chain.hip (layers 2 + 3 of SA1's 4 -> 64 -> 64 -> 128 MLP chained in registers, BatchNorm
    statistics and pooled extrema as in-lane reductions) == the layer-by-layer kernels: both raw
    outputs, both layers' BatchNorm coefficients and running statistics, the pooled tensor, the
    arg-max (pytorch_utils.py:14-39,70-124, pointnet2_modules.py:256-262).  Negative gammas and
    duplicated columns (pool ties: the first index wins) included.  (The chain against float64, per
    channel and edge by edge: tests/test_sa1_train_gpu.py.)"""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(b * 100 + ns)
    x = (torch.randn(b, 4, m, ns, generator=g) * 1.5 + 0.4).to(DEV)
    x[:, :, :, 5] = x[:, :, :, 2]          # ties inside a group
    x[:, :, 1::3, ns - 1] = x[:, :, 1::3, 0]
    w0 = (torch.randn(64, 4, generator=g) * 0.7).to(DEV)
    w1 = (torch.randn(64, 64, generator=g) / 8).to(DEV)
    w2 = (torch.randn(128, 64, generator=g) / 8).to(DEV)

    def bn(c):
        gamma = (torch.rand(c, generator=g) + 0.5)
        gamma[::5] *= -1
        return [gamma.to(DEV), (torch.randn(c, generator=g) * 0.3).to(DEV)]

    g0, g1, g2 = bn(64), bn(64), bn(128)
    assert K.chain_lin4_supported(w0, w1, w2, x, ns)

    def run(chain):
        rs = [[torch.zeros(c, device=DEV), torch.ones(c, device=DEV)] for c in (64, 64, 128)]
        mom = K.first4_moments(x)
        c0 = K.first4_bn(mom, x.numel() // 4, w0, g0[0], g0[1], rs[0][0], rs[0][1], 0.1, 1e-5)
        if chain:
            y1, c1, y2, c2, ext = K.chain_lin4_forward(
                x, w0, (c0[2], c0[3]), (w1, g1[0], g1[1], rs[1][0], rs[1][1], 0.1, 1e-5),
                (w2, g2[0], g2[1], rs[2][0], rs[2][1], 0.1, 1e-5))
        else:
            y1, *c1 = K.gemm_forward_bn_lin4(w1, x, w0, (c0[2], c0[3]), g1[0], g1[1], rs[1][0], rs[1][1], 0.1, 1e-5)
            y2, *rest = K.gemm_forward_bn(w2, y1, (c1[2], c1[3]), g2[0], g2[1], rs[2][0], rs[2][1], 0.1, 1e-5,
                                          pool=True)
            c2, ext = rest[:4], rest[4]
            assert ext is not None
        pooled, argmax, ymax = K.pool_from_extrema(ext, c2[2], c2[3])
        return y1, list(c1), y2, list(c2), pooled, argmax, ymax, rs

    got, want = run(True), run(False)
    close(got[0], want[0], 1e-5)
    close(got[2], want[2], 2e-5)
    for a_, b_ in zip(got[1] + got[3], want[1] + want[3]):
        close(a_, b_, 2e-5)
    for (a0, a1), (b0, b1) in zip(got[7], want[7]):
        close(a0, b0, 2e-5); close(a1, b1, 2e-5)
    close(got[4], want[4], 2e-5)
    close(got[6], want[6], 2e-5)
    # the arg-max: where the two paths differ the rivals are within rounding of one another
    diff = got[5] != want[5]
    assert float(diff.float().mean()) < 2e-3
    y2w = want[2]
    pick = lambda idx: torch.gather(y2w, 3, idx.long().unsqueeze(-1)).squeeze(-1)  # noqa: E731
    assert float((pick(got[5]) - pick(want[5])).abs().max()) <= 2e-5 * float(y2w.abs().max())
    # exact ties (duplicated columns): the FIRST index wins in both
    assert not bool((got[5] == 5).any()) and not bool((want[5] == 5).any())


@pytest.mark.parametrize("b,m,ns", [(8, 1024, 32), (3, 200, 32), (12, 1024, 32), (8, 512, 16), (5, 256, 16),
                                     (1, 2048, 16), (16, 1024, 32), (2, 1000, 32)])
def test_pooled_forward_without_its_raw_output(b, m, ns, monkeypatch):
    """csrc/mlp_pool_fwd256.hip: the max-pooled 128 -> 256 layer (conv(1x1) of pytorch_utils.py:70-124 on
    relu(bn(y2)), BatchNorm statistics, max over nsample of pointnet2_modules.py:256-262) leaving
    statistics + extrema only == float64 torch, and == the tiled kernel that stores y3: values, the
    FIRST index on exact ties, negative BatchNorm weights (the smallest raw value wins there)."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(b * 7 + m + ns)
    y2 = (torch.randn(b, 128, m, ns, generator=g) * 1.3 + 0.2).to(DEV)
    y2[:, :, :, 3] = y2[:, :, :, 1]  # duplicated columns, as ball_query pads: pool ties
    y2[:, :, ::7, ns - 1] = y2[:, :, ::7, 0]
    w3 = (torch.randn(256, 128, generator=g) / 11).to(DEV)
    g2, be2 = (torch.rand(128, generator=g) + 0.5).to(DEV), (torch.randn(128, generator=g) * 0.3).to(DEV)
    g3 = torch.rand(256, generator=g) + 0.5
    g3[::5] *= -1
    g3 = g3.to(DEV)
    be3 = (torch.randn(256, generator=g) * 0.3).to(DEV)
    z = lambda c: (torch.zeros(c, device=DEV), torch.ones(c, device=DEV))  # noqa: E731
    c2 = K.bn_coefficients(y2, g2, be2, *z(128), 0.1, 1e-5, True)
    if not K.forward_pool_supported(w3, y2, (c2[2], c2[3])):
        pytest.skip("no pooled epilogue at this size")
    rs = z(256)
    none, mean, invstd, sc, sh, ext = K.gemm_forward_bn(w3, y2, (c2[2], c2[3]), g3, be3, *rs, 0.1, 1e-5,
                                                        pool=True, store=False)
    assert none is None
    a2 = torch.relu(y2.double() * c2[2].double().view(1, -1, 1, 1) + c2[3].double().view(1, -1, 1, 1))
    y64 = torch.einsum("ck,bkmn->bcmn", w3.double(), a2)
    rng = float(y64.abs().max())
    mean64, var64 = y64.mean(dim=(0, 2, 3)), y64.var(dim=(0, 2, 3), unbiased=False)
    assert float((mean.double() - mean64).abs().max()) <= 1e-6 * rng
    assert float((invstd.double() * (var64 + 1e-5).sqrt() - 1).abs().max()) <= 1e-5
    n = y64.numel() // 256
    assert float((rs[0].double() - 0.1 * mean64).abs().max()) <= 1e-6 * rng  # running statistics updated
    assert float((rs[1].double() - (0.9 + 0.1 * var64 * n / (n - 1))).abs().max()) <= 1e-5 * float(var64.max())
    sign = torch.where(g3 < 0, -1.0, 1.0).double().view(1, -1, 1)
    best64 = (y64 * sign.unsqueeze(-1)).max(dim=3).values * sign
    assert float((ext[0].double() - best64).abs().max()) <= 2e-6 * rng
    idx = ext[1].view(torch.int32).long()
    assert int(idx.min()) >= 0 and int(idx.max()) < ns
    picked = torch.gather(y64, 3, idx.unsqueeze(-1)).squeeze(-1)
    assert float((picked - best64).abs().max()) <= 2e-6 * rng  # (a rival within rounding at worst)
    # exact ties: columns 1 and 3 are equal everywhere, columns 0 and ns - 1 in every 7th group
    assert not bool((idx == 3).any())
    assert not bool((idx[:, :, ::7] == ns - 1).any())
    # the form that also stores y3 (the same kernel): identical statistics and extrema, y3 == float64
    y3, mean_s, invstd_s, _, _, ext_s = K.gemm_forward_bn(w3, y2, (c2[2], c2[3]), g3, be3, *z(256), 0.1, 1e-5,
                                                          pool=True)
    assert torch.equal(ext_s, ext) and torch.equal(mean_s, mean) and torch.equal(invstd_s, invstd)
    assert float((y3.double() - y64).abs().max()) <= 2e-6 * rng
    # against the tiled kernel (gemm_nn2_kernel with its pooled epilogue)
    monkeypatch.setenv("MLP_POOL_FWD256", "0")
    y3_t, mean_t, invstd_t, _, _, ext_t = K.gemm_forward_bn(w3, y2, (c2[2], c2[3]), g3, be3, *z(256), 0.1, 1e-5,
                                                            pool=True)
    monkeypatch.delenv("MLP_POOL_FWD256")
    assert float((y3 - y3_t).abs().max()) <= 2e-6 * rng
    assert float((ext[0] - ext_t[0]).abs().max()) <= 2e-6 * rng
    assert float((ext[1].view(torch.int32) != ext_t[1].view(torch.int32)).float().mean()) < 1e-3
    pooled, argmax, ymax = K.pool_from_extrema(ext, sc, sh)
    want = torch.relu(y3 * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).max(dim=3).values
    assert float((pooled - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("b,c,r,training", [(8, 256, 1024, True), (16, 256, 1024, True), (8, 128, 256, True),
                                              (3, 259, 1000, True), (1, 64, 4096, True), (8, 256, 1024, False),
                                              (5, 128, 36, True), (12, 32, 1024, True)])
def test_batchnorm_per_channel_forms(b, c, r, training, monkeypatch):
    """csrc/mlp_bn.hip, the small layers' forms (one workgroup per channel, no partials, no tickets):
    training statistics + coefficients (nn.BatchNorm2d of pytorch_utils.py:14-39), the backward sums and
    dy of BatchNorm + ReLU == float64 torch and == the ticket forms (MLP_BN_CHANNEL_FORM=0)."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(b * 3 + c + r)
    y = (torch.randn(b, c, r, generator=g) * 1.7 + 0.4).to(DEV)
    dz = torch.randn(b, c, r, generator=g).to(DEV)
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::4] *= -1
    gamma, beta = gamma.to(DEV), (torch.randn(c, generator=g) * 0.3).to(DEV)

    def run():
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, rm, rv, 0.1, 1e-5, True)
        dy, dgamma, dbeta = K.bn_relu_backward(y, dz, gamma, scale, shift, mean, invstd, training)
        dg2, db2, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, training)
        return [t.clone() for t in (mean, invstd, scale, shift, rm, rv, dy, dgamma, dbeta, dg2, db2, coef)]

    new = run()
    monkeypatch.setenv("MLP_BN_CHANNEL_FORM", "0")
    old = run()
    monkeypatch.delenv("MLP_BN_CHANNEL_FORM")
    y64, dz64 = y.double(), dz.double()
    mean64, var64 = y64.mean(dim=(0, 2)), y64.var(dim=(0, 2), unbiased=False)
    n = b * r
    assert float((new[0].double() - mean64).abs().max()) <= 1e-6 * float(y64.abs().max())
    assert float((new[1].double() * (var64 + 1e-5).sqrt() - 1).abs().max()) <= 1e-5
    assert float((new[4].double() - 0.1 * mean64).abs().max()) <= 1e-6 * float(y64.abs().max())
    assert float((new[5].double() - (0.9 + 0.1 * var64 * n / max(n - 1, 1))).abs().max()) <= 1e-5 * float(var64.max())
    sc64, sh64 = new[2].double().view(1, -1, 1), new[3].double().view(1, -1, 1)
    g64 = torch.where(y64 * sc64 + sh64 > 0, dz64, torch.zeros_like(dz64))
    xhat = (y64 - new[0].double().view(1, -1, 1)) * new[1].double().view(1, -1, 1)
    s1, s2 = g64.sum(dim=(0, 2)), (g64 * xhat).sum(dim=(0, 2))
    tol = 3e-6 * float(g64.abs().sum(dim=(0, 2)).max())
    assert float((new[8].double() - s1).abs().max()) <= tol and float((new[7].double() - s2).abs().max()) <= tol
    a64 = gamma.double() * new[1].double()
    c1 = s1 / n if training else torch.zeros_like(s1)
    c2 = s2 / n if training else torch.zeros_like(s2)
    dy64 = a64.view(1, -1, 1) * (g64 - c1.view(1, -1, 1) - xhat * c2.view(1, -1, 1))
    assert float((new[6].double() - dy64).abs().max()) <= 1e-5 * float(dy64.abs().max())
    for i, (p, q) in enumerate(zip(new, old)):  # the two forms against one another
        assert float((p - q).abs().max()) <= 1e-5 * float(q.abs().max()) + 1e-7, i
    assert torch.equal(new[7], new[9]) and torch.equal(new[8], new[10])  # sums-only launch == sums + dy launch


@pytest.mark.parametrize("b,m,ns,pool,direct", [(8, 1024, 32, False, False), (8, 512, 64, True, False),
                                                 (8, 512, 16, True, False), (4, 512, 32, True, False),
                                                 (3, 1000, 32, False, False), (8, 512, 16, False, True),
                                                 (5, 256, 64, True, False), (16, 512, 16, False, False)])
def test_forward_128_channels_t_form(b, m, ns, pool, direct):
    """csrc/mlp_gemm.hip (the tiled kernels): a 128 -> 128 layer (conv(1x1) of pytorch_utils.py:70-124 on
    relu(bn(x)) or on x itself, BatchNorm statistics, optionally the max over nsample of
    pointnet2_modules.py:256-262 with nsample 16 / 32 / 64) == float64 torch."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(b * 5 + m + ns)
    x = (torch.randn(b, 128, m, ns, generator=g) * 1.3 + 0.2).to(DEV)
    x[:, :, :, 3] = x[:, :, :, 1]  # pool ties
    x[:, :, ::7, ns - 1] = x[:, :, ::7, 0]
    # (the weight at an odd 4-byte offset for some shapes, as inside the optimizer's flat parameter buffer)
    flat = torch.zeros(128 * 128 + 3, device=DEV)
    off = (b + m) % 4
    w = flat[off:off + 128 * 128].view(128, 128)
    w.copy_((torch.randn(128, 128, generator=g) / 11).to(DEV))
    g2, be2 = (torch.rand(128, generator=g) + 0.5).to(DEV), (torch.randn(128, generator=g) * 0.3).to(DEV)
    g3 = torch.rand(128, generator=g) + 0.5
    g3[::5] *= -1
    g3 = g3.to(DEV)
    be3 = (torch.randn(128, generator=g) * 0.3).to(DEV)
    z = lambda c: (torch.zeros(c, device=DEV), torch.ones(c, device=DEV))  # noqa: E731
    c2 = K.bn_coefficients(x, g2, be2, *z(128), 0.1, 1e-5, True)
    coeff = None if direct else (c2[2], c2[3])
    out = K.gemm_forward_bn(w, x, coeff, g3, be3, *z(128), 0.1, 1e-5, pool=pool)
    a2 = x.double() if direct else torch.relu(x.double() * c2[2].double().view(1, -1, 1, 1) +
                                              c2[3].double().view(1, -1, 1, 1))
    y64 = torch.einsum("ck,bkmn->bcmn", w.double(), a2)
    rng = float(y64.abs().max())
    mean64, var64 = y64.mean(dim=(0, 2, 3)), y64.var(dim=(0, 2, 3), unbiased=False)
    assert float((out[0].double() - y64).abs().max()) <= 2e-6 * rng
    assert float((out[1].double() - mean64).abs().max()) <= 1e-6 * rng
    assert float((out[2].double() * (var64 + 1e-5).sqrt() - 1).abs().max()) <= 1e-5
    if pool:
        ext = out[5]
        assert (ext is None) == (off != 0)  # (the pooled epilogue wants aligned rows)
    if pool and off == 0:
        sign = torch.where(g3 < 0, -1.0, 1.0).double().view(1, -1, 1)
        best64 = (y64 * sign.unsqueeze(-1)).max(dim=3).values * sign
        assert float((ext[0].double() - best64).abs().max()) <= 2e-6 * rng
        idx = ext[1].view(torch.int32).long()
        assert int(idx.min()) >= 0 and int(idx.max()) < ns
        picked = torch.gather(y64, 3, idx.unsqueeze(-1)).squeeze(-1)
        assert float((picked - best64).abs().max()) <= 2e-6 * rng
        assert not bool((idx == 3).any()) and not bool((idx[:, :, ::7] == ns - 1).any())  # exact ties: the first


@pytest.mark.parametrize("b,m,ns,kin,mout", [(8, 256, 64, 64, 128), (4, 300, 32, 64, 128), (2, 1024, 16, 64, 128),
                                             (3, 77, 64, 64, 128), (8, 1024, 32, 128, 256),
                                             (2, 512, 16, 128, 256), (3, 200, 32, 128, 256),
                                             (1, 128, 16, 128, 256), (3, 512, 16, 128, 256),
                                             (8, 512, 16, 128, 256), (8, 256, 16, 128, 256),
                                             (5, 256, 16, 128, 256), (4, 512, 32, 128, 256),
                                             (3, 1024, 16, 128, 256), (16, 1024, 32, 128, 256)])
def test_pooled_backward_from_the_gram_matrix(b, m, ns, kin, mout, monkeypatch):
    """csrc/mlp_pool_gram.hip: the backward of a max-pooled last layer y3 = w3 . relu(bn(y2)) WITHOUT
    y3 (dy3 = q y3 + p + S: da2 = (W3^T diag(q) W3) a2 + W3^T p + W3^T S, dW3 = diag(q) W3 (a2 a2^T) +
    p (sum a2)^T + S a2^T) == the one-pass kernel that rebuilds dy3 from the stored y3: gradient
    w.r.t. the layer's input, weight gradient, BatchNorm-backward sums of the layer below
    (autograd of pytorch_utils.py:14-39,70-124 + pointnet2_modules.py:256-262).
    (The (128, 64) pass against float64 at every kind of chunk range: tests/test_pool_gram128_gpu.py.)"""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    monkeypatch.setenv("MLP_POOL_GRAM256_MIN_CHUNKS", "64")  # (the product takes this path from 4096 chunks on)
    g = torch.Generator().manual_seed(b * 31 + m + ns)
    y2 = (torch.randn(b, kin, m, ns, generator=g) * 1.3 + 0.2).to(DEV)
    y2[:, :, :, 3] = y2[:, :, :, 1]  # duplicated columns, as ball_query pads: pool ties
    w3 = (torch.randn(mout, kin, generator=g) / kin ** 0.5).to(DEV)

    def bn(c):
        gamma = torch.rand(c, generator=g) + 0.5
        gamma[::5] *= -1
        return gamma.to(DEV), (torch.randn(c, generator=g) * 0.3).to(DEV)

    g2, be2 = bn(kin)
    g3, be3 = bn(mout)
    z = lambda c: (torch.zeros(c, device=DEV), torch.ones(c, device=DEV))  # noqa: E731
    c2 = K.bn_coefficients(y2, g2, be2, *z(kin), 0.1, 1e-5, True)
    assert K.pool_gram_supported(w3, y2, ns)
    y3, mean3, invstd3, sc3, sh3, ext = K.gemm_forward_bn(w3, y2, (c2[2], c2[3]), g3, be3, *z(mout), 0.1, 1e-5,
                                                          pool=True)
    if ext is None:
        pooled, argmax, ymax = K.bn_relu_pool(y3, sc3, sh3)
    else:
        pooled, argmax, ymax = K.pool_from_extrema(ext, sc3, sh3)
    if K.forward_pool_supported(w3, y2, (c2[2], c2[3])):
        # the forward pass that stores no raw output leaves the same statistics and extrema
        none, mean3n, invstd3n, sc3n, sh3n, extn = K.gemm_forward_bn(w3, y2, (c2[2], c2[3]), g3, be3, *z(mout),
                                                                     0.1, 1e-5, pool=True, store=False)
        assert none is None
        if tuple(w3.shape) == (128, 64):  # the same kernel with its store removed
            assert torch.equal(extn, ext) and torch.equal(mean3n, mean3) and torch.equal(sc3n, sc3)
        else:  # (256,128): a kernel of its own (csrc/mlp_pool_fwd256.hip), another summation order
            rng = float(y3.abs().max())
            assert float((extn[0] - ext[0]).abs().max()) <= 2e-6 * rng
            assert float((mean3n - mean3).abs().max()) <= 1e-6 * rng
            assert float((invstd3n / invstd3 - 1).abs().max()) <= 1e-5
            differ = extn[1].view(torch.int32) != ext[1].view(torch.int32)
            assert float(differ.float().mean()) < 1e-3  # (rivals within rounding of one another)
    dpooled = torch.randn(b, mout, m, generator=g).to(DEV)
    dgamma, dbeta, coef3 = K.bn_relu_pool_backward_stats(y3, dpooled, argmax, ymax, g3, sc3, sh3, mean3,
                                                         invstd3, True)
    want = K.gemm_backward_fused(w3, y2, (c2[2], c2[3]),
                                 pooled=(y3, dpooled, argmax, sc3, sh3, mean3, invstd3, coef3),
                                 xstats=(c2[0], c2[1], g2, True))
    if want is None:
        want_dx = K.gemm_dgrad(w3, pooled=(y3, dpooled, argmax, sc3, sh3, mean3, invstd3, coef3))
        want_dw = K.gemm_wgrad(mout, kin, y2, (c2[2], c2[3]),
                               pooled=(y3, dpooled, argmax, sc3, sh3, mean3, invstd3, coef3))
        want_below = K.bn_relu_backward_stats(y2, want_dx.contiguous(), g2, c2[2], c2[3], c2[0], c2[1], True)
    else:
        want_dx, want_dw, want_below = want
        if want_below is None:  # (256,128): the one-pass kernel leaves no sums for the layer below
            want_below = K.bn_relu_backward_stats(y2, want_dx.view_as(y2).contiguous(), g2, c2[2], c2[3], c2[0],
                                                  c2[1], True)
    dgamma_g, dbeta_g, coef_g = K.bn_relu_pool_backward_stats(None, dpooled, argmax, ymax, g3, sc3, sh3,
                                                              mean3, invstd3, True, ns=ns)
    assert torch.equal(coef_g, coef3) and torch.equal(dgamma_g, dgamma)
    # the size threshold is the forward's decision alone: restored before the backward (most of these
    # shapes are below it), the backward must still run
    monkeypatch.delenv("MLP_POOL_GRAM256_MIN_CHUNKS")
    dx, dw, below = K.pool_gram_backward(w3, y2, c2, g2, coef3, (mean3, invstd3, sc3, sh3), dpooled, argmax,
                                         ymax, ns, True)
    rel = lambda a_, b_: float((a_ - b_).norm() / (b_.norm() + 1e-20))  # noqa: E731
    print("gram backward vs stored-y3 backward: dx %.2e dw %.2e dgamma %.2e dbeta %.2e coef %.2e" % (
        rel(dx, want_dx.view_as(dx)), rel(dw, want_dw), rel(below[0], want_below[0]),
        rel(below[1], want_below[1]), rel(below[2], want_below[2])))
    close(dx, want_dx.view_as(dx), 3e-5)
    assert rel(dx, want_dx.view_as(dx)) < 2e-5
    close(dw, want_dw, 1e-4)
    assert rel(dw, want_dw) < 1e-4
    # the BatchNorm-backward sums of the layer below are sums of ~1e5 terms of both signs of THIS pass's
    # dx: measured against a float64 evaluation of those sums (the other path's sums belong to ITS dx,
    # 3e-7 away element by element -- after the cancellation that is 1e-5 of the sum)
    xh = (y2.double() - c2[0].double().view(1, -1, 1, 1)) * c2[1].double().view(1, -1, 1, 1)
    gate = (y2.double() * c2[2].double().view(1, -1, 1, 1) + c2[3].double().view(1, -1, 1, 1)) > 0
    gd = torch.where(gate, dx.double(), torch.zeros((), dtype=torch.float64, device=DEV))
    assert _rel(below[0], (gd * xh).sum(dim=(0, 2, 3))) < 3e-6 and _rel(below[1], gd.sum(dim=(0, 2, 3))) < 3e-6
    assert _rel(below[0], want_below[0]) < 1e-3 and _rel(below[1], want_below[1]) < 1e-3
    close(below[2][:, 0], want_below[2][:, 0], 1e-6)  # (a = gamma * invstd: no sum)


@pytest.mark.parametrize("b,m,ns", [(8, 2048, 64), (2, 256, 32)])
def test_sa1_chain_and_gram_vs_float64_torch(b, m, ns):
    """An INDEPENDENT check of the round-5 SA1 kernels at the step's real shape (B = 8, m = 2048,
    ns = 64: VERDICT r5 weak item 13): csrc/mlp_chain.hip's forward (layers 2 + 3 chained in
    registers, last raw output not stored) and csrc/mlp_pool_gram.hip's backward (from the Gram
    matrix of the layer's input) against a float64 torch evaluation of the reference's module --
    Conv2d 1x1 (no bias) + BatchNorm2d (batch statistics) + ReLU, three times, then the max over
    nsample (pytorch_utils.py:14-39,70-124, pointnet2_modules.py:256-262) -- and its autograd.
    (The forward alone at small shapes, every nsample, stored outputs and per-channel measures:
    tests/test_sa1_train_gpu.py; the backward alone, on inputs no kernel prepares and under a measured
    bound: tests/test_pool_gram128_gpu.py.)"""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(7 * b + m + ns)
    x = (torch.randn(b, 4, m, ns, generator=g) * 1.5 + 0.4).to(DEV)
    w = [(torch.randn(64, 4, generator=g) * 0.7).to(DEV), (torch.randn(64, 64, generator=g) / 8).to(DEV),
         (torch.randn(128, 64, generator=g) / 8).to(DEV)]

    def bn(c):
        gamma = torch.rand(c, generator=g) + 0.5
        gamma[::5] *= -1
        return gamma.to(DEV), (torch.randn(c, generator=g) * 0.3).to(DEV)

    gb = [bn(64), bn(64), bn(128)]
    eps = 1e-5
    assert K.chain_lin4_supported(w[0], w[1], w[2], x, ns) and K.pool_gram_supported(w[2], x.new_empty(b, 64, m, ns), ns)
    rs = [[torch.zeros(c, device=DEV), torch.ones(c, device=DEV)] for c in (64, 64, 128)]
    c0 = K.first4_bn(K.first4_moments(x), x.numel() // 4, w[0], gb[0][0], gb[0][1], rs[0][0], rs[0][1], 0.1, eps)
    y1, c1, y2, c2, ext = K.chain_lin4_forward(
        x, w[0], (c0[2], c0[3]), (w[1], gb[1][0], gb[1][1], rs[1][0], rs[1][1], 0.1, eps),
        (w[2], gb[2][0], gb[2][1], rs[2][0], rs[2][1], 0.1, eps), store_last=False)
    assert y2 is None, "the last raw output was stored"
    pooled, argmax, ymax = K.pool_from_extrema(ext, c2[2], c2[3])
    dpooled = torch.randn(b, 128, m, generator=g).to(DEV)
    dgamma2, dbeta2, coef2 = K.bn_relu_pool_backward_stats(None, dpooled, argmax, ymax, gb[2][0], c2[2], c2[3],
                                                           c2[0], c2[1], True, ns=ns)
    da1, dw2, below = K.pool_gram_backward(w[2], y1, c1, gb[1][0], coef2, c2, dpooled, argmax, ymax, ns, True)

    # ---- the same module in float64 ----
    W = [t.double().requires_grad_(True) for t in w]
    G = [(ga.double().requires_grad_(True), be.double().requires_grad_(True)) for ga, be in gb]

    def layer(inp, i):
        y = torch.einsum("oc,bcmn->bomn", W[i], inp)
        mean = y.mean(dim=(0, 2, 3), keepdim=True)
        var = y.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        a = torch.relu((y - mean) / torch.sqrt(var + eps) * G[i][0].view(1, -1, 1, 1) + G[i][1].view(1, -1, 1, 1))
        return y, mean.flatten(), (1.0 / torch.sqrt(var + eps)).flatten(), a

    y0_64, _, _, a0 = layer(x.double(), 0)
    y1_64, mean1, inv1, a1 = layer(a0, 1)
    a1.retain_grad()
    y2_64, mean2, inv2, a2 = layer(a1, 2)
    pooled64, argmax64 = a2.max(dim=3)
    # forward: raw output of layer 2 of the module, both layers' batch statistics, the pooled tensor
    close(y1, y1_64, 2e-5)
    close(c1[0], mean1, 2e-5); close(c1[1], inv1, 2e-5)
    close(c2[0], mean2, 2e-5); close(c2[1], inv2, 2e-5)
    close(pooled, pooled64, 2e-5)
    # the arg-max: where it differs from float64's the rivals are within fp32 rounding of one another
    flips = argmax.long() != argmax64
    assert float(flips.float().mean()) < 1e-3, float(flips.float().mean())
    at_kernel = torch.gather(a2, 3, argmax.long().unsqueeze(-1)).squeeze(-1)
    assert float((pooled64 - at_kernel).abs().max()) <= 2e-5 * float(pooled64.abs().max())
    # backward through the KERNEL's winners (a flipped winner is another, equally valid subgradient)
    (at_kernel * dpooled.double()).sum().backward()
    n_flips = int(flips.sum())
    rel = lambda a_, b_: float((a_.double() - b_).norm() / (b_.norm() + 1e-300))  # noqa: E731
    print("chain + gram vs float64 [%d x %d x %d]: %d arg-max flips of %d; da1 %.2e dw2 %.2e dgamma2 %.2e "
          "dbeta2 %.2e dgamma1 %.2e dbeta1 %.2e" % (b, m, ns, n_flips, flips.numel(), rel(da1, a1.grad),
                                                    rel(dw2, W[2].grad), rel(dgamma2, G[2][0].grad),
                                                    rel(dbeta2, G[2][1].grad), rel(below[0], G[1][0].grad),
                                                    rel(below[1], G[1][1].grad)))
    # (ReLU gates within rounding of 0 may differ between fp32 and float64: single elements)
    assert rel(da1, a1.grad) < 2e-4
    d = (da1.double() - a1.grad).abs()
    assert float((d > 1e-4 * float(a1.grad.abs().max())).float().mean()) < 1e-4
    assert rel(dw2, W[2].grad) < 2e-4
    assert rel(dgamma2, G[2][0].grad) < 2e-4 and rel(dbeta2, G[2][1].grad) < 2e-4
    assert rel(below[0], G[1][0].grad) < 5e-4 and rel(below[1], G[1][1].grad) < 5e-4


def test_reductions_on_two_streams_at_once():
    """The BatchNorm reductions finalize in their last workgroup through per-channel ticket
    counters; launches that may overlap must not share counters, and the counters are the
    CALLER's (include/mlp_hip.h `tickets`; nothing in the library is keyed by stream).  Two streams
    run statistics + backward sums of different tensors back to back, forty times each, every
    stream with its own array: every result equals the one computed alone, the arrays are zero
    afterwards."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(5)
    cases = []
    for c, r in ((64, 40000), (128, 9000)):
        y = (torch.randn(4, c, r, generator=g) * 1.5 + 0.3).to(DEV)
        dz = torch.randn(4, c, r, generator=g).to(DEV)
        gamma = (torch.rand(c, generator=g) + 0.5).to(DEV)
        beta = (torch.randn(c, generator=g) * 0.3).to(DEV)
        cases.append((y, dz, gamma, beta, K.new_tickets(c, DEV)))

    def work(case):
        y, dz, gamma, beta, tickets = case
        rm, rv = torch.zeros_like(gamma), torch.ones_like(gamma)
        mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, rm, rv, 0.1, 1e-5, True, tickets)
        dgamma, dbeta, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, True, tickets)
        return [mean, invstd, dgamma, dbeta, coef]

    alone = [[t.clone() for t in work(cs)] for cs in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = [[], []]
    for _ in range(40):
        for si, st in enumerate(streams):
            with torch.cuda.stream(st):
                got[si].append(work(cases[si]))
    torch.cuda.synchronize()
    for si in range(2):
        assert int(cases[si][4].abs().sum()) == 0
        for res in got[si]:
            for a, b in zip(res, alone[si]):
                assert torch.equal(a, b)
    # a wrong array is refused, not read
    y, dz, gamma, beta, _ = cases[0]
    with pytest.raises(RuntimeError, match="tickets"):
        K.bn_coefficients(y, gamma, beta, None, None, 0.1, 1e-5, True, torch.zeros(8, dtype=torch.int32, device=DEV))


def test_two_modules_replayed_side_by_side_on_any_streams():
    """Two shared-MLP modules (a student's and a teacher's), each captured into a HIP graph -- one
    of them on torch's default capture stream, the handle every capture without a stream argument
    uses -- and replayed side by side on two streams, 32 times: every replay returns exactly what
    the module returns alone.  Each module owns the counters of its reductions
    (_mlp_ext.tickets_of): in round 5 two graphs captured on one stream handle shared an array
    keyed by that stream and corrupted each other's statistics."""
    load_pkg()
    pu = importlib.import_module("pointnet2.pytorch_utils")
    torch.manual_seed(21)
    mods = [pu.SharedMLP([16, 64, 64, 128], bn=True).to(DEV).train() for _ in range(2)]
    xs = [torch.randn(4, 16, 256, 32, device=DEV) for _ in range(2)]

    def state(m):
        return [b.clone() for b in m.buffers()]

    def restore(m, saved):
        for b, v in zip(m.buffers(), saved):
            b.copy_(v)

    with torch.no_grad():
        for m, x in zip(mods, xs):  # lazy initialisation outside the captures
            m.forward_pooled(x)
    saved = [state(m) for m in mods]
    alone = []
    with torch.no_grad():
        for m, x, sv in zip(mods, xs, saved):
            restore(m, sv)
            alone.append(m.forward_pooled(x).clone())
    tickets = [m._pn2_tickets for m in mods]
    assert tickets[0].data_ptr() != tickets[1].data_ptr()
    capture_streams = [torch.cuda.graph.default_capture_stream, torch.cuda.Stream()]
    graphs, outs = [], []
    torch.cuda.synchronize()
    for m, x, cs in zip(mods, xs, capture_streams):
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g, stream=cs):
            outs.append(m.forward_pooled(x))
        graphs.append(g)
    replay_streams = [torch.cuda.Stream(), torch.cuda.graph.default_capture_stream]
    for _ in range(32):
        for m, sv in zip(mods, saved):
            restore(m, sv)
        torch.cuda.synchronize()
        for g, st in zip(graphs, replay_streams):
            with torch.cuda.stream(st):
                g.replay()
        torch.cuda.synchronize()
        for o, a, t in zip(outs, alone, tickets):
            assert torch.equal(o, a)
            assert int(t.abs().sum()) == 0


def test_queued_weight_gradient_reductions_equal_immediate_ones():
    """Inside deferred_weight_reductions() the partial-sum reductions of gemm_wgrad /
    gemm_backward_fused are queued and run as one launch at exit (more than one when the queue of
    40 fills): every dw is bit-identical to the one reduced at once, data gradients are untouched,
    and outside the context the launches are immediate again."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(11)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(DEV)

    plain = []  # (m, k, x, dy): stand-alone weight gradients of assorted shapes
    for m, k, r in ((64, 4, 4096), (128, 64, 3000), (256, 259, 1000), (128, 131, 2048), (2, 3, 64),
                    (256, 256, 512), (79, 128, 1024)):
        plain.append((m, k, rnd(2, k, r), rnd(2, m, r)))

    def fused_case(b, m, k, groups, ns):  # both gradients of one layer from one pass over (y, dz)
        w = rnd(m, k) / k ** 0.5
        x, y, dz = rnd(b, k, groups, ns), rnd(b, m, groups, ns), rnd(b, m, groups, ns)
        gamma = (torch.rand(m, generator=g) + 0.5).to(DEV)
        beta = rnd(m) * 0.3
        rm, rv = torch.zeros(m, device=DEV), torch.ones(m, device=DEV)
        mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, rm, rv, 0.1, 1e-5, True)
        _, _, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, True)
        return w, x, (y, dz, scale, shift, mean, invstd, coef)

    fused = [fused_case(2, 128, 131, 40, 32), fused_case(5, 128, 259, 26, 16)]

    def run():
        out = []
        for rep in range(7):  # 7 x (7 + 2) = 63 queued reductions: the queue of 40 overflows once
            for m, k, x, dy in plain:
                out.append(K.gemm_wgrad(m, k, x, None, dy=dy))
            for w, x, fly in fused:
                both = K.gemm_backward_fused(w, x, None, fly=fly)
                assert both is not None
                out.extend([both[0], both[1]])
        return out

    ref = [t.clone() for t in run()]
    with K.deferred_weight_reductions():
        got = run()
    torch.cuda.synchronize()
    assert len(got) == len(ref) and len(ref) >= 49
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    again = run()  # immediate launches after the context
    for a, b in zip(again, ref):
        assert torch.equal(a, b)


def test_deferred_reductions_with_a_frozen_weight():
    """A SharedMLP whose middle convolution is frozen (requires_grad False) under
    deferred_weight_reductions(): autograd drops that layer's dw as soon as the backward returns
    it, the queued reduction still writes it at the flush -- so the tensor must stay allocated
    until then (the caching allocator would otherwise hand the block to a live tensor
    and the flush would overwrite it).  Everything else equals the immediate form bit for bit."""
    pt = _mods()
    K = importlib.import_module("pointnet2._mlp_ext")
    torch.manual_seed(11)
    mlp = pt.SharedMLP([128, 128, 128, 256], bn=True).to(DEV).train()
    mlp[1].conv.weight.requires_grad_(False)
    x0 = torch.randn(4, 128, 512, 32, device=DEV)
    wgt = torch.randn(4, 256, 512, device=DEV)

    def run(deferred):
        x = x0.clone().requires_grad_(True)
        mlp.zero_grad()
        out = mlp.forward_pooled(x)
        held = []
        with K.deferred_weight_reductions(deferred):
            (out * wgt).sum().backward()
            # allocations while the reductions are still queued: each would receive the block of a
            # dropped dw if it had been freed (128 x 128 floats = the frozen layer's gradient)
            held = [torch.full((128, 128), 7.0, device=DEV) for _ in range(64)]
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in held)
        grads = [p.grad.clone() for p in mlp.parameters() if p.grad is not None]
        return [x.grad.clone()] + grads

    want, got = run(False), run(True)
    assert mlp[1].conv.weight.grad is None
    assert len(want) == len(got)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("b,n,c,m,ns,widths,scale,training", [
    (2, 2048, 128, 1024, 32, (128, 128, 256), 1.0, True),
    (3, 1024, 256, 512, 16, (128, 128, 256), 1.0 / 0.8, True),
    (2, 512, 256, 256, 16, (128, 128, 256), 1.0, True),
    (2, 1000, 64, 300, 8, (64, 128), 2.5, True),
    (2, 2048, 128, 1024, 32, (128, 128, 256), 1.0, False)])
def test_pregathered_first_layer_vs_grouped(b, n, c, m, ns, widths, scale, training):
    """SharedMLP.forward_pregathered (first layer applied over the N points, its output gathered:
    csrc/mlp_pregather.hip) == forward_pooled of the grouped tensor the reference forms
    (pointnet2_utils.py:335-358 + pytorch_utils.py:14-39): pooled output, gradients of the features
    and of every parameter, running statistics."""
    import copy
    pt = _mods()
    ext = importlib.import_module("pointnet2._ext")
    g = torch.Generator().manual_seed(b * 1000 + n + c + m + ns)
    xyzs = [(torch.rand(b, n, 3, generator=torch.Generator().manual_seed(3)) * 4 - 2).to(DEV)
            .requires_grad_(True) for _ in range(2)]
    pick = torch.randperm(n, generator=g)[:m].to(DEV)
    news = [x[:, pick] for x in xyzs]  # centroids are points of the cloud: their gradient flows on
    xyz, new_xyz = xyzs[1], news[1]
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(DEV)
    idx[:, :, 1] = idx[:, :, 0]  # repeated members, as ball_query pads
    inverse = ext.group_inverse(idx, n)
    assert inverse is not None
    feats = [torch.randn(b, c, n, generator=g).to(DEV).requires_grad_(True) for _ in range(2)]
    feats[1].data.copy_(feats[0].data)
    torch.manual_seed(5)
    mlp_a = pt.SharedMLP([c + 3] + list(widths), bn=True).to(DEV)
    for mod in mlp_a.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
    mlp_b = copy.deepcopy(mlp_a)
    mlp_a.train(training); mlp_b.train(training)
    mlp_64 = _f64_twin(mlp_a)
    assert mlp_b.pregather_ok(xyz, new_xyz, feats[1], m, ns)
    # the reference's grouped tensor
    li = idx.long()
    gx = torch.gather(xyzs[0].transpose(1, 2).unsqueeze(2).expand(b, 3, m, n), 3,
                      li.unsqueeze(1).expand(b, 3, m, ns))
    gx = (gx - news[0].transpose(1, 2).unsqueeze(-1)) * scale
    gf = torch.gather(feats[0].unsqueeze(2).expand(b, c, m, n), 3, li.unsqueeze(1).expand(b, c, m, ns))
    out_a = mlp_a.forward_pooled(torch.cat([gx, gf], dim=1).contiguous())
    out_b = mlp_b.forward_pregathered(xyz, new_xyz, feats[1], idx, inverse, scale)
    close(out_b, out_a, 2e-5)
    if training:
        dout = torch.randn(out_a.shape, generator=g).to(DEV)
        out_a.backward(dout)
        out_b.backward(dout)
        # the two forwards differ in the last ulp, so a pre-activation within rounding of 0 can flip
        # its ReLU mask and a max over nsample pick another near-tied sample (as in
        # test_fused_chain_vs_sequential): almost every element agrees tightly, the sums in L2
        d = (feats[1].grad - feats[0].grad).abs()
        assert float((d > 5e-4 * max(1.0, float(feats[0].grad.abs().max()))).float().mean()) < 2e-3
        # ... measured against the float64 evaluation of the reference's formulation (_grad_bound:
        # each fp32 path has its own flipped gates; neither is the other's truth)
        x64 = xyzs[0].detach().double().requires_grad_(True)
        f64 = feats[0].detach().double().requires_grad_(True)
        gx64 = torch.gather(x64.transpose(1, 2).unsqueeze(2).expand(b, 3, m, n), 3,
                            li.unsqueeze(1).expand(b, 3, m, ns))
        gx64 = (gx64 - x64[:, pick].transpose(1, 2).unsqueeze(-1)) * scale
        gf64 = torch.gather(f64.unsqueeze(2).expand(b, c, m, n), 3, li.unsqueeze(1).expand(b, c, m, ns))
        z64 = torch.nn.Sequential.forward(mlp_64, torch.cat([gx64, gf64], dim=1))
        torch.max(z64, dim=3)[0].backward(dout.double())
        _grad_bound(feats[1].grad, feats[0].grad, f64.grad)
        # scatter over idx + (through the centroids) minus the group sums
        _grad_bound(xyzs[1].grad, xyzs[0].grad, x64.grad)
        for (na, pa), (nb, pb), (nc, pc) in zip(mlp_a.named_parameters(), mlp_b.named_parameters(),
                                                mlp_64.named_parameters()):
            _grad_bound(pb.grad, pa.grad, pc.grad)
    for (na, ba), (nb, bb) in zip(mlp_a.named_buffers(), mlp_b.named_buffers()):
        close(bb.float(), ba.float(), 2e-5)


@pytest.mark.parametrize("b,m,k,r", [(8, 256, 256, 1024), (8, 256, 512, 512), (3, 128, 128, 256),
                                     (2, 79, 128, 256), (8, 128, 259, 768), (2, 259, 256, 1000),
                                     (1, 64, 20, 36)])
def test_small_backward_pair_vs_two_gemms(b, m, k, r):
    """One launch for the data gradient and the weight gradient of a small layer
    (mlp_gemm_backward_small) == gemm_dgrad + gemm_wgrad: the same two kernel bodies, so the same
    bits for dq; dw within the tolerance of its (differently sliced) partial sums.  Gradient
    operand given or formed on the fly, input direct or relu(bn(.)), with and without dq."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(m + k + r)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = torch.randn(b, k, r, generator=g).to(DEV)
    y = torch.randn(b, m, r, generator=g).to(DEV)
    dz = torch.randn(b, m, r, generator=g).to(DEV)
    gamma = (torch.rand(m, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(m, generator=g) * 0.3).to(DEV)
    mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, torch.zeros(m, device=DEV),
                                                   torch.ones(m, device=DEV), 0.1, 1e-5, True)
    _, _, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, True)
    fly = (y, dz, scale, shift, mean, invstd, coef)
    xc = ((torch.rand(k, generator=g) + 0.5).to(DEV), (torch.randn(k, generator=g) * 0.2).to(DEV))
    for grad in (dict(fly=fly), dict(dy=dz)):
        for xcoeff in (None, xc):
            pair = K.gemm_backward_small(w, x, xcoeff, **grad)
            assert pair is not None, "shape not in the small regime"
            dx, dw = pair
            want_dx = K.gemm_dgrad(w, **grad).view_as(x)
            want_dw = K.gemm_wgrad(m, k, x, xcoeff, **grad)
            assert torch.equal(dx, want_dx)
            close(dw, want_dw, 1e-5)
            none, dw_only = K.gemm_backward_small(w, x, xcoeff, need_dx=False, **grad)
            assert none is None
            assert torch.equal(dw_only, dw)


@pytest.mark.parametrize("b,m,k,r", [(8, 256, 512, 1024), (8, 259, 256, 1024), (3, 79, 128, 256),
                                     (2, 128, 131, 100), (1, 64, 20, 36), (8, 128, 259, 768)])
def test_small_gemms_from_weight_images(b, m, k, r, monkeypatch):
    """The small layers' kernels with their weight taken from the bf16 images that ONE launch
    writes for a whole set of weights (mlp_weight_images_build; WeightImages) == the same kernels
    splitting the fp32 weight tile in every workgroup: forward (plain and BatchNorm + ReLU'ed
    input) and the pair launch of the backward (data gradient through the TRANSPOSED image, weight
    gradient untouched), bit for bit; ragged rows / columns / reduction lengths (zero padding of
    the images); a weight that is not in the set, a layer outside the small regime and an update
    of the weight without refresh() behave as documented."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    g = torch.Generator().manual_seed(m * 7 + k + r)
    w = (torch.randn(m, k, 1, 1, generator=g) / k ** 0.5).to(DEV)
    other = (torch.randn(m, k, 1, generator=g) / k ** 0.5).to(DEV)
    w2 = w.reshape(m, k)
    x = torch.randn(b, k, r, generator=g).to(DEV)
    dy = torch.randn(b, m, r, generator=g).to(DEV)
    ck = ((torch.rand(k, generator=g) + 0.5).to(DEV), (torch.randn(k, generator=g) * 0.3).to(DEV))
    images = K.WeightImages([w, torch.ones(7, device=DEV), other])   # (1-D tensors are skipped)
    assert images.n == 2
    images.refresh()
    want = [K.gemm_forward(w2, x), K.gemm_forward(w2, x, ck), K.gemm_backward_small(w2, x, ck, dy=dy),
            K.gemm_backward_small(w2, x, None, dy=dy)]
    with K.weight_images(images):
        assert K._image_of(w2, b, r) is not None
        got = [K.gemm_forward(w2, x), K.gemm_forward(w2, x, ck), K.gemm_backward_small(w2, x, ck, dy=dy),
               K.gemm_backward_small(w2, x, None, dy=dy)]
        stranger = torch.randn(m, k, device=DEV)
        assert K._image_of(stranger, b, r) is None
        assert torch.equal(K.gemm_forward(stranger, x), K.gemm_forward(stranger, x))
        assert K._image_of(w2, 64, 1024) is None          # 65536 columns: not the small kernel
    assert K._image_of(w2, b, r) is None                    # outside the context
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for (dx_g, dw_g), (dx_w, dw_w) in zip(got[2:], want[2:]):
        assert torch.equal(dx_g, dx_w) and torch.equal(dw_g, dw_w)
    # the images are a snapshot: an in-place update shows only after refresh()
    w.mul_(2.0)
    with K.weight_images(images):
        stale = K.gemm_forward(w2, x)
        images.refresh()
        fresh = K.gemm_forward(w2, x)
    assert torch.equal(stale, want[0]) and torch.equal(fresh, K.gemm_forward(w2, x))


@pytest.mark.parametrize("training", [True, False])
def test_first_layer_commuted_with_the_interpolation(training, monkeypatch):
    """SharedMLP.forward_pooled_interp (no-grad passes of the IoU branch, grid_conv_module.py:87-110):
    W0 . cat([rel, interpolate(f)]) computed as interpolate(W0[:, 3:] . f) + W0[:, :3] . rel -- the
    GEMM over the 1024 seeds instead of the 16384 grid points, one kernel for interpolation + the
    coordinate rows (pn2_three_interpolate_affine, also checked alone against torch) -- == the shared
    MLP on the materialised input: pooled features to 1e-4 of their range, running statistics too."""
    P = _mods()
    ext = importlib.import_module("pointnet2._ext")
    g = torch.Generator().manual_seed(5)
    b, c, s, k, g3 = 3, 256, 1024, 40, 64
    n = k * g3
    f = torch.randn(b, c, s, generator=g).to(DEV)
    idx = torch.randint(0, s, (b, n, 3), generator=g, dtype=torch.int32).to(DEV)
    wt = torch.rand(b, n, 3, generator=g)
    wt = (wt / wt.sum(-1, keepdim=True)).to(DEV)
    rel = torch.randn(b, 3, n, generator=g).to(DEV)
    # the kernel alone
    z = torch.randn(b, 128, s, generator=g).to(DEV)
    aw = torch.randn(128, 3, generator=g).to(DEV)
    got = ext.three_interpolate_affine(z, idx, wt, aw, rel)
    gathered = torch.gather(z.unsqueeze(2).expand(b, 128, n, s), 3, idx.long().unsqueeze(1).expand(b, 128, n, 3))
    want = (gathered * wt.unsqueeze(1)).sum(-1) + torch.einsum("cd,bdn->bcn", aw, rel)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    # the module
    torch.manual_seed(0)
    outs = []
    for commuted in (False, True):
        torch.manual_seed(0)
        mlp = P.SharedMLP([c + 3, 128, 128, 128], bn=True).to(DEV)
        mlp.train(training)
        with torch.no_grad():
            if commuted:
                assert mlp.interp_first_ok(f, idx)
                out = mlp.forward_pooled_interp(f, idx, wt, rel, k, g3)
            else:
                feats = torch.empty(b, 3 + c, n, device=DEV)
                feats[:, :3] = rel
                ext.three_interpolate_into(f, idx, wt, feats, 3)
                out = mlp.forward_pooled(feats.view(b, 3 + c, k, g3))
        outs.append((out, [bb.clone() for bb in mlp.buffers()]))
    (o0, b0), (o1, b1) = outs
    assert o0.shape == o1.shape == (b, 128, k)
    assert float((o0 - o1).abs().max()) <= 1e-4 * max(1.0, float(o0.abs().max()))
    for x, y in zip(b0, b1):
        assert torch.allclose(x.float(), y.float(), rtol=1e-4, atol=1e-5)
    # a pass that records gradients: same output, and the parameters' gradients agree (the layer's
    # input is then formed in the backward pass, for the weight gradient); features WITH a gradient
    # are declined (that gradient would need the scatter form)
    assert not mlp.interp_first_ok(f.clone().requires_grad_(True), idx)
    if training:
        probe = torch.randn(b, 128, k, generator=g).to(DEV)
        grads = []
        for commuted in (False, True):
            torch.manual_seed(0)
            mlp = P.SharedMLP([c + 3, 128, 128, 128], bn=True).to(DEV).train()
            if commuted:
                assert mlp.interp_first_ok(f, idx)
                out = mlp.forward_pooled_interp(f, idx, wt, rel, k, g3)
            else:
                feats = torch.empty(b, 3 + c, n, device=DEV)
                feats[:, :3] = rel
                ext.three_interpolate_into(f, idx, wt, feats, 3)
                out = mlp.forward_pooled(feats.view(b, 3 + c, k, g3))
            (out * probe).sum().backward()
            grads.append({name: p_.grad.clone() for name, p_ in mlp.named_parameters()})
        whole = float(torch.sqrt(sum((v.double() ** 2).sum() for v in grads[0].values())))
        for name in grads[0]:
            err = float((grads[0][name] - grads[1][name]).norm()) / max(0.01 * whole, float(grads[0][name].norm()))
            assert err <= 2e-3, (name, err)
    monkeypatch.setenv("PN2_INTERP_FIRST", "0")
    with torch.no_grad():
        assert not mlp.interp_first_ok(f, idx)
