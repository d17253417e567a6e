"""The 512-thread, two-role form of the (128,128) one-pass backward (csrc/mlp_bwd_x6.h): waves 0-3
compute the data gradient and the BatchNorm sums, waves 4-7 the weight gradient, the staging is
shared out between them.  The four forms of the kernel (gradient operand from (y, dz) or from the
pooled tensors, with and without the sums of the layer below) at the shapes a role split can break,
against a float64 two-GEMM reference, and twice with bit-equal results.

The forms with the sums go through gemm_backward_fused; the wrapper always asks for the sums of a
relu(bn(.)) input, so the forms without them go through the library handle of the same module
(mlp_gemm_backward_fused with a null stats_part).  Tolerances: those of
test_gpu_mlp.py::test_fused_backward_vs_two_gemms (1e-5 dx, 2e-5 dw, 2e-5 the sums)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(a, b, tol):  # (the measure of test_gpu_mlp.py: max error against the reference's range)
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    scale = max(1.0, float(np.abs(b).max()))
    assert np.abs(a - b).max() <= tol * scale, float(np.abs(a - b).max())


def _fused_without_sums(K, w, x, xcoeff, xstats, fly=None, pooled=None):
    """mlp_gemm_backward_fused with stats_part = NULL: the kernel's forms without the sums"""
    b, k = x.shape[0], x.shape[1]
    m = w.shape[0]
    r = x.numel() // (b * k)
    p, q = K._grad_operand(fly=fly, pooled=pooled), K._input_operand(x, xcoeff, xstats)
    assert K._lib.mlp_gemm_backward_fused_supported(b, m, k, r, p.mode, 1, p.ns)
    dx = torch.empty_like(x)
    dw = torch.empty((m, k), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws = torch.empty(max(int(K._lib.mlp_gemm_backward_fused_workspace_floats(b, m, k, r)), 1),
                         dtype=torch.float32, device=x.device)
        K._L.check(K._lib.mlp_gemm_backward_fused(b, m, k, r, w.data_ptr(), ctypes.byref(p),
                                                  ctypes.byref(q), dx.data_ptr(), dw.data_ptr(),
                                                  ws.data_ptr(), None, K._stream(x)),
                   "mlp_gemm_backward_fused")
        torch.cuda.synchronize()
    return dx, dw, None


# (b, groups, ns, pooled): total chunks = b * groups * ns / 32, workgroups = min(CUs, chunks / 8)
SHAPES = [
    (3, 25, 32, False),    # 75 chunks over 9 workgroups: ranges of 9 (odd: the last chunk on buffer 0
                           # only) and a last range of 3; chunks that cross into the next cloud
    (1, 64, 32, False),    # b = 1 at the smallest size the kernel accepts (64 chunks, 8 per workgroup)
    (2, 165, 32, False),   # 330 chunks: more than one per CU, not a multiple of the workgroup count
    (3, 50, 16, True),     # pooled, ns = 16 (two groups per chunk), 75 chunks over 9 workgroups
    (1, 64, 32, True),     # pooled, ns = 32 (one group per chunk), b = 1, the smallest size
    (3, 13, 64, True),     # pooled, ns = 64 (two chunks per group), 78 chunks over 9 workgroups
    (2, 330, 16, True),    # pooled, ns = 16, 330 chunks
]


@pytest.mark.parametrize("sums", [True, False])
@pytest.mark.parametrize("b,groups,ns,pooled", SHAPES)
def test_bwd_x6_roles_vs_float64(b, groups, ns, pooled, sums):
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    m = k = 128
    g = torch.Generator().manual_seed(1000 * b + 10 * groups + ns + int(pooled))
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
        dy, _, _ = K.bn_relu_pool_backward(y, dpooled, argmax, ymax, gamma, scale, shift, mean,
                                           invstd, True)
        kw = dict(pooled=(y, dpooled, argmax, scale, shift, mean, invstd, coef))
    else:
        dz = torch.randn(b, m, groups, ns, generator=g).to(DEV)
        _, _, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, True)
        dy, _, _ = K.bn_relu_backward(y, dz, gamma, scale, shift, mean, invstd, True)
        kw = dict(fly=(y, dz, scale, shift, mean, invstd, coef))
    xgamma = (torch.rand(k, generator=g) + 0.5).to(DEV)
    xbeta = (torch.randn(k, generator=g) * 0.3).to(DEV)
    xmean, xinv, xscale, xshift = K.bn_coefficients(x, xgamma, xbeta, torch.zeros(k, device=DEV),
                                                    torch.ones(k, device=DEV), 0.1, 1e-5, True)
    xcoeff, xstats = (xscale, xshift), (xmean, xinv, xgamma, True)

    def run():
        if sums:
            return K.gemm_backward_fused(w, x, xcoeff, xstats=xstats, **kw)
        return _fused_without_sums(K, w, x, xcoeff, xstats, **kw)

    both = run()
    assert both is not None, "shape not routed to the fused kernel"
    dx, dw, below = both
    assert (below is not None) == sums

    # float64 reference: the two GEMMs on the materialised gradient operand and relu(bn(x))
    r = groups * ns
    dy64 = dy.double().view(b, m, r)
    x64 = x.double().view(b, k, r)
    q64 = torch.relu(x64 * xscale.double().view(1, k, 1) + xshift.double().view(1, k, 1))
    want_dx = torch.einsum("mk,bmr->bkr", w.double(), dy64)
    want_dw = torch.einsum("bmr,bkr->mk", dy64, q64)
    close(dx.view(b, k, r), want_dx, 1e-5)
    close(dw, want_dw, 2e-5)
    if sums:  # the layer below's BatchNorm-backward sums from (x, dx)
        # the gate of the kernels, fmaf(x, scale, shift) > 0: in float64 the product is exact and the
        # sum keeps its sign, so this is the same decision
        z64 = x64 * xscale.double().view(1, k, 1) + xshift.double().view(1, k, 1)
        g64 = torch.where(z64 > 0, want_dx, torch.zeros_like(want_dx))
        xhat = (x64 - xmean.double().view(1, k, 1)) * xinv.double().view(1, k, 1)
        close(below[1], g64.sum(dim=(0, 2)), 2e-5)
        close(below[0], (g64 * xhat).sum(dim=(0, 2)), 2e-5)
        _, _, want_coef = K.bn_relu_backward_stats(x, want_dx.float().view_as(x).contiguous(), xgamma,
                                                   xscale, xshift, xmean, xinv, True)
        close(below[2], want_coef, 2e-5)

    # twice: bit-equal (fixed chunk ranges, fixed order of every sum)
    dx2, dw2, below2 = run()
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)
    if sums:
        for a, c in zip(below, below2):
            assert torch.equal(a, c)
