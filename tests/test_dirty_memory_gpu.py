"""Every kernel binding on poisoned allocations (tests/dirty_memory.py): the operation is called once
clean and once under each of the three fills -- NaN, +3e38, -3e38 in every float tensor the
binding allocates for itself (outputs, workspaces, partials; 0xFF in the listed bf16 / double byte
buffers) -- from the same seeded inputs and the same in-place state.  Then

  * the helper has poisoned at least one allocation,
  * every float element of every result is finite and below 1e30 (inputs are N(0,1)-scale),
  * the three poisoned results equal each other and the clean result BIT FOR BIT.

A result that depends on memory nobody initialised -- a tail tile that is not stored, a partial an
idle workgroup never wrote but the reduction reads, a padded row multiplied by zero, an accumulator
that relies on arriving as zero -- fails one of the three.  The poison block wraps only the call
under test; inputs are built outside it; nothing is captured into a graph.

Bit-equality is relaxed only for the operations below, whose kernels add floats with atomics in an
order the hardware chooses; each is held to the tolerance its existing test uses against its
reference (rtol 0), with the clean result as the reference:

  operation (shape class)                     kernel                                  tolerance (existing test)
  three_interpolate_grad, m > 1024            three_interpolate_grad_kernel           1e-4 * max(1, |want|.max())
  three_interpolate_grad_from, m > 1024       (global atomicAdd, pn2_interp.hip)        test_gpu_ops.py test_three_interpolate_every_kernel_vs_oracle
  group_points_grad (unsorted)                group_points_grad_lds_kernel (LDS       1e-4
                                              atomicAdd from 16 waves),                 test_gpu_ops.py test_group_vs_oracle
                                              group_points_grad_lds_range_kernel,
                                              group_points_grad_kernel (global
                                              atomicAdd, n > 40960 and few rows)
  gather_points_grad                          gather_points_grad_kernel (global       1e-4
                                              atomicAdd, pn2_sampling.hip)              test_gpu_ops.py test_gather_golden

Documented unwritten regions of a returned tensor: none.  (three_interpolate_into /
three_interpolate_rows_into write a channel slice of a tensor the CALLER passes in -- "written into
channels [channel0, channel0 + C) of the preallocated contiguous (B, C_total, n) tensor `out`",
pointnet2/_ext.py -- the rest of that tensor is the caller's and is compared like everything else:
it must come back untouched.)
"""
import importlib
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_pkg
from dirty_memory import FILLS, FILL_IDS, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ATOL_ATOMIC = {  # name in the table above -> atol(clean result)
    "three_interpolate_grad": lambda want: 1e-4 * max(1.0, float(want.abs().max())),
    "group_points_grad": lambda want: 1e-4,
    "gather_points_grad": lambda want: 1e-4,
}


def _K():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


def _E():
    load_pkg()
    return importlib.import_module("pointnet2._ext")


def _flatten(out, into=None):
    """the tensors of a nested result, in order (None and non-tensors keep their place)"""
    into = [] if into is None else into
    if isinstance(out, torch.Tensor):
        into.append(out)
    elif isinstance(out, (tuple, list)):
        for o in out:
            _flatten(o, into)
    elif isinstance(out, dict):
        for key in sorted(out):
            _flatten(out[key], into)
    elif hasattr(out, "partials"):  # _mlp_ext.GatedSums
        into.append(out.partials)
    else:
        into.append(out)
    return into


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def _sane(results, label):
    for i, t in enumerate(results):
        if isinstance(t, torch.Tensor) and t.is_floating_point() and t.numel():
            d = t.detach()
            assert bool(torch.isfinite(d).all()), "%s: result %d is not finite" % (label, i)
            assert float(d.abs().max()) < 1e30, "%s: result %d holds %g" % (label, i, float(d.abs().max()))


def _same(got, want, label, atomic):
    assert len(got) == len(want), label
    for i, (a, b) in enumerate(zip(got, want)):
        if not isinstance(b, torch.Tensor):
            assert a == b or (isinstance(b, float) and math.isnan(a) and math.isnan(b)), (label, i)
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (label, i)
        if atomic is not None and b.is_floating_point():
            atol = ATOL_ATOMIC[atomic](b.detach())
            err = float((a.detach() - b.detach()).abs().max()) if b.numel() else 0.0
            assert err <= atol, "%s: result %d off by %g > %g" % (label, i, err, atol)
        else:
            differ = int((_bits(a) != _bits(b)).sum())
            assert differ == 0, "%s: result %d differs from the clean run in %d of %d elements" % (
                label, i, differ, b.numel())


def check(call, state=None, atomic=None, min_count=1, min_bytes=0):
    """call(*state()) clean, then under each fill; state() builds the tensors the operation updates in
    place afresh (outside the poison block), and call returns them with its results.  min_bytes: the
    least number of allow-listed byte / int16 buffers (dirty_memory.BYTE_SITES) the call must have had
    filled with 0xFF -- a site whose size function moved out of the allocating function would
    otherwise stop being poisoned unnoticed."""
    def once(fill):
        args = state() if state is not None else ()
        if fill is None:
            out = call(*args)
            count = byte_count = None
        else:
            with poisoned(fill) as p:
                out = call(*args)
            count, byte_count = p.count, p.byte_count
        torch.cuda.synchronize()
        return _flatten(out), count, byte_count

    clean, _, _ = once(None)
    _sane(clean, "clean")
    for fill, name in zip(FILLS, FILL_IDS):
        got, count, byte_count = once(fill)
        assert count >= min_count, "fill %s: nothing was poisoned" % name
        assert byte_count >= min_bytes, "fill %s: %d of %d listed byte buffers poisoned" % (name, byte_count, min_bytes)
        _sane(got, "fill " + name)
        _same(got, clean, "fill " + name, atomic)
    return clean


def _gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * (31 ** i) for i, s in enumerate(seed)) % (2 ** 31))


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(DEV)


def _bn_params(g, c, negative=True):
    gamma = torch.rand(c, generator=g) + 0.5
    if negative:
        gamma[::5] *= -1
    return gamma.to(DEV), (torch.randn(c, generator=g) * 0.3).to(DEV)


def _running(c):
    return lambda: (torch.zeros(c, device=DEV), torch.ones(c, device=DEV))


def test_check_catches_what_it_is_for():
    """the procedure itself on three stand-in bindings in plain torch: a tail that is not stored, an
    accumulator that relies on its buffer arriving as zero, an extremum seeded from the buffer (the
    case NaN alone would miss: fmax drops it) -- each must fail; the correct one must pass"""
    x = _randn(_gen(1), 64)

    def tail_not_stored():
        out = torch.empty(64, device=DEV)
        out[:63] = x[:63]
        return out

    def accumulates():
        out = torch.empty_like(x)
        out += x
        return out

    def seeded_extremum():
        best = x.new_empty(1)
        return torch.fmax(best, x.max())

    def correct():
        out = torch.empty_like(x)
        out.copy_(x)
        return out

    for broken in (tail_not_stored, accumulates, seeded_extremum):
        with pytest.raises(AssertionError):
            check(broken)
    check(correct)


# =================================== tier 1: the operator matrix ===================================
GEMM_SHAPES = [(1, 3, 7, 33), (3, 259, 128, 96), (1, 65, 300, 777), (2, 131, 259, 1024), (2, 300, 128, 256)]


def _gemm_operands(b, m, k, r):
    g = _gen(b, m, k, r)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = _randn(g, b, k, r)
    xc = ((torch.rand(k, generator=g) + 0.5).to(DEV), _randn(g, k, scale=0.3))
    y, dz = _randn(g, b, m, r), _randn(g, b, m, r)
    sc, sh = (torch.rand(m, generator=g) + 0.5).to(DEV), _randn(g, m, scale=0.3)
    mu, istd = _randn(g, m, scale=0.2), (torch.rand(m, generator=g) + 0.5).to(DEV)
    coef = torch.stack([torch.rand(m, generator=g) + 0.5, torch.randn(m, generator=g) * 0.1,
                        torch.randn(m, generator=g) * 0.1], dim=1).contiguous().to(DEV)
    return w, x, xc, (y, dz, sc, sh, mu, istd, coef)


def _pooled_operand(K, g, b, m, groups, ns):
    """a pooled layer's gradient operand (y, dpooled, argmax, scale, shift, mean, invstd, coef) + ymax"""
    y = _randn(g, b, m, groups, ns)
    gamma, beta = _bn_params(g, m, negative=False)
    rm, rv = _running(m)()
    mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, rm, rv, 0.1, 1e-5, True)
    _, argmax, ymax = K.bn_relu_pool(y, scale, shift)
    dpooled = _randn(g, b, m, groups)
    _, _, coef = K.bn_relu_pool_backward_stats(y, dpooled, argmax, ymax, gamma, scale, shift, mean, invstd, True)
    return (y, dpooled, argmax, scale, shift, mean, invstd, coef), ymax


def _fly_operand(K, g, b, m, *cols):
    y, dz = _randn(g, b, m, *cols), _randn(g, b, m, *cols)
    gamma, beta = _bn_params(g, m, negative=False)
    rm, rv = _running(m)()
    mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, rm, rv, 0.1, 1e-5, True)
    _, _, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, True)
    return (y, dz, scale, shift, mean, invstd, coef)


@pytest.mark.parametrize("small", [True, False], ids=["small-tile", "big-tile"])
@pytest.mark.parametrize("b,m,k,r", GEMM_SHAPES)
def test_gemm_forward_dgrad_wgrad(b, m, k, r, small, monkeypatch):
    monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "1000000000" if small else "0")
    K = _K()
    w, x, xc, fly = _gemm_operands(b, m, k, r)
    dy = fly[1]
    check(lambda: K.gemm_forward(w, x))
    check(lambda: K.gemm_forward(w, x, xc))
    check(lambda: K.gemm_dgrad(w, dy=dy))
    check(lambda: K.gemm_dgrad(w, fly=fly))
    check(lambda: K.gemm_wgrad(m, k, x, None, dy=dy))
    check(lambda: K.gemm_wgrad(m, k, x, xc, fly=fly))


@pytest.mark.parametrize("small", [True, False], ids=["small-tile", "big-tile"])
@pytest.mark.parametrize("b,m,k,groups,ns", [(1, 3, 7, 11, 3), (3, 259, 128, 6, 16), (1, 65, 300, 111, 7),
                                             (2, 131, 259, 32, 32), (2, 300, 128, 16, 16)])
def test_gemm_dgrad_wgrad_pooled_operand(b, m, k, groups, ns, small, monkeypatch):
    """(the GEMM shapes above with r = groups * ns)"""
    monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "1000000000" if small else "0")
    K = _K()
    g = _gen(b, m, k, groups, ns)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = _randn(g, b, k, groups, ns)
    xc = ((torch.rand(k, generator=g) + 0.5).to(DEV), _randn(g, k, scale=0.3))
    op, _ = _pooled_operand(K, g, b, m, groups, ns)
    check(lambda: K.gemm_dgrad(w, pooled=op))
    check(lambda: K.gemm_wgrad(m, k, x, None, pooled=op))
    check(lambda: K.gemm_wgrad(m, k, x, xc, pooled=op))


@pytest.mark.parametrize("b,m,k,r", [(2, 79, 128, 256), (8, 259, 256, 1024)])
def test_gemm_forward_from_weight_images(b, m, k, r):
    """the images themselves are built in poisoned memory too (0xFF bytes: the int16 buffer is listed)"""
    K = _K()
    g = _gen(b, m, k, r)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x, dy = _randn(g, b, k, r), _randn(g, b, m, r)
    xc = ((torch.rand(k, generator=g) + 0.5).to(DEV), _randn(g, k, scale=0.3))

    def run():
        images = K.WeightImages([w])
        images.refresh()
        with K.weight_images(images):
            assert K._image_of(w, b, r) is not None
            return (K.gemm_forward(w, x), K.gemm_forward(w, x, xc), K.gemm_backward_small(w, x, xc, dy=dy),
                    K.gemm_backward_small(w, x, None, dy=dy))

    check(run, min_count=2, min_bytes=1)


@pytest.mark.parametrize("epilogue", [True, False], ids=["pairs-epilogue", "default-regime"])
@pytest.mark.parametrize("b,m,k,groups,ns", [(2, 64, 4, 32, 32), (3, 128, 64, 16, 32), (1, 96, 131, 520, 32)])
def test_gemm_forward_bn(b, m, k, groups, ns, epilogue, monkeypatch):
    """default-regime: below 16384 columns the layer is a small GEMM followed by the statistics pass;
    pairs-epilogue (MLP_SMALL_GEMM_COLS=0): the statistics, and the pooled extrema, leave the GEMM's
    epilogue as per-tile partials, as they do at the network's sizes"""
    if epilogue:
        monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "0")
    K = _K()
    g = _gen(b, m, k, groups, ns)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = _randn(g, b, k, groups, ns)
    coeff = None if k == 4 else ((torch.rand(k, generator=g) + 0.5).to(DEV), _randn(g, k, scale=0.3))
    gamma, beta = _bn_params(g, m)
    flat = x.view(b, k, groups * ns)
    scratch = 1 if epilogue else 0  # (mlp_bn_finalize_pairs' scratch of doubles: a listed byte buffer)
    check(lambda rm, rv: (K.gemm_forward_bn(w, flat, coeff, gamma, beta, rm, rv, 0.1, 1e-5), rm, rv), _running(m),
          min_bytes=scratch)
    check(lambda rm, rv: (K.gemm_forward_bn(w, x, coeff, gamma, beta, rm, rv, 0.1, 1e-5, pool=True), rm, rv),
          _running(m), min_bytes=scratch)
    if K.forward_pool_supported(w, x, coeff):
        def run(rm, rv):
            out = K.gemm_forward_bn(w, x, coeff, gamma, beta, rm, rv, 0.1, 1e-5, pool=True, store=False)
            return out, K.pool_from_extrema(out[5], out[3], out[4]), rm, rv
        check(run, _running(m), min_bytes=1)
    else:
        assert not epilogue or (m, k) != (128, 64), "the pooled epilogue should cover this layer"


def _lin4_module(g):
    w0 = (torch.randn(64, 4, generator=g) * 0.7).to(DEV)
    w1 = (torch.randn(64, 64, generator=g) / 8).to(DEV)
    w2 = (torch.randn(128, 64, generator=g) / 8).to(DEV)
    return w0, w1, w2, _bn_params(g, 64), _bn_params(g, 64), _bn_params(g, 128)


@pytest.mark.parametrize("b,m,ns", [(2, 256, 32), (2, 1024, 16)])
def test_virtual_first_layer_forward_and_chain(b, m, ns, monkeypatch):
    monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "0")  # (2 x 256 x 32 columns are not above the default threshold)
    K = _K()
    g = _gen(b, m, ns)
    x = _randn(g, b, 4, m, ns, scale=1.5, shift=0.4)
    w0, w1, w2, g0, g1, g2 = _lin4_module(g)
    assert K.lin4_supported(w0, w1, x) and K.chain_lin4_supported(w0, w1, w2, x, ns)
    mom = K.first4_moments(x)
    c0 = K.first4_bn(mom, x.numel() // 4, w0, g0[0], g0[1], None, None, 0.1, 1e-5)
    state = lambda: _running(64)() + _running(128)()  # noqa: E731
    check(lambda rm1, rv1, rm2, rv2: (
        K.gemm_forward_bn_lin4(w1, x, w0, (c0[2], c0[3]), g1[0], g1[1], rm1, rv1, 0.1, 1e-5), rm1, rv1), state,
        min_bytes=1)
    for kw in (dict(), dict(store_last=False), dict(store=False)):
        def run(rm1, rv1, rm2, rv2):
            out = K.chain_lin4_forward(x, w0, (c0[2], c0[3]), (w1, g1[0], g1[1], rm1, rv1, 0.1, 1e-5),
                                       (w2, g2[0], g2[1], rm2, rv2, 0.1, 1e-5), **kw)
            return out, K.pool_from_extrema(out[4], out[3][2], out[3][3]), rm1, rv1, rm2, rv2
        check(run, state, min_bytes=1)  # (the module's weight image)


def _x6_case(K, b, groups, ns, pooled, m=128, k=128, xbn=True):
    g = _gen(b, groups, ns, int(pooled), m, k)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = _randn(g, b, k, groups, ns)
    if pooled:
        op, _ = _pooled_operand(K, g, b, m, groups, ns)
        kw = dict(pooled=op)
    else:
        kw = dict(fly=_fly_operand(K, g, b, m, groups, ns))
    xcoeff = xstats = None
    if xbn:
        xgamma, xbeta = _bn_params(g, k, negative=False)
        xmean, xinv, xscale, xshift = K.bn_coefficients(x, xgamma, xbeta, *_running(k)(), 0.1, 1e-5, True)
        xcoeff, xstats = (xscale, xshift), (xmean, xinv, xgamma, True)
    return w, x, xcoeff, xstats, kw


@pytest.mark.parametrize("sums", [True, False])
@pytest.mark.parametrize("b,groups,ns,pooled", [(3, 25, 32, False), (1, 64, 32, False), (2, 165, 32, False),
                                                (3, 50, 16, True), (3, 13, 64, True)])
def test_gemm_backward_fused_128(b, groups, ns, pooled, sums):
    """the first four rows and the (3,13,64,True) row of tests/test_bwd_x6_roles.py SHAPES: ranges of 9
    chunks with a last range of 3, chunks that cross into the next cloud"""
    from test_bwd_x6_roles import _fused_without_sums
    K = _K()
    w, x, xcoeff, xstats, kw = _x6_case(K, b, groups, ns, pooled)
    if sums:
        def run():
            out = K.gemm_backward_fused(w, x, xcoeff, xstats=xstats, **kw)
            assert out is not None and out[2] is not None
            return out
    else:
        def run():
            return _fused_without_sums(K, w, x, xcoeff, xstats, **kw)
    check(run)


def test_gemm_backward_fused_other_shapes():
    K = _K()
    w, x, xcoeff, xstats, kw = _x6_case(K, 5, 26, 16, False, m=128, k=259, xbn=False)

    def dw_only():
        out = K.gemm_backward_fused(w, x, None, need_dx=False, **kw)
        assert out is not None and out[0] is None
        return out
    check(dw_only)
    check(lambda: K.gemm_backward_fused(w, x, None, **kw))
    w, x, xcoeff, xstats, kw = _x6_case(K, 2, 40, 64, False, m=64, k=64)

    def with_sums():
        out = K.gemm_backward_fused(w, x, xcoeff, xstats=xstats, **kw)
        assert out is not None and out[2] is not None
        return out
    check(with_sums)


def test_gemm_backward_fused_virtual_first_layer(monkeypatch):
    """qmode 4: the layer below is the virtual 4 -> 64 layer; the gated sums and the weight gradient
    wgrad_first4_from_gated forms of them"""
    monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "0")
    K = _K()
    b, m, ns = 2, 256, 32
    g = _gen(b, m, ns, 4)
    x = _randn(g, b, 4, m, ns, scale=1.5, shift=0.4)
    w0, w1, _, g0, g1, _ = _lin4_module(g)
    mom = K.first4_moments(x)
    c0 = K.first4_bn(mom, x.numel() // 4, w0, g0[0], g0[1], None, None, 0.1, 1e-5)
    y1, mean1, inv1, sc1, sh1 = K.gemm_forward_bn_lin4(w1, x, w0, (c0[2], c0[3]), g1[0], g1[1], None, None, 0.1, 1e-5)
    dz = _randn(g, b, 64, m, ns)
    _, _, coef1 = K.bn_relu_backward_stats(y1, dz, g1[0], sc1, sh1, mean1, inv1, True)
    fly = (y1, dz, sc1, sh1, mean1, inv1, coef1)

    def run():
        out = K.gemm_backward_fused(w1, x, (c0[2], c0[3]), fly=fly, xstats=(c0[0], c0[1], g0[0], True), lin_w=w0)
        assert out is not None
        gated, dw, below = out
        return out, K.wgrad_first4_from_gated(w0, gated, c0[0], c0[1], below[2], mom)
    check(run)


@pytest.mark.parametrize("b,m,k,r", [(3, 128, 128, 256), (2, 79, 128, 256)])
def test_gemm_backward_small_and_both(b, m, k, r):
    K = _K()
    g = _gen(b, m, k, r)
    w = (torch.randn(m, k, generator=g) / k ** 0.5).to(DEV)
    x = _randn(g, b, k, r)
    xc = ((torch.rand(k, generator=g) + 0.5).to(DEV), _randn(g, k, scale=0.2))
    fly = _fly_operand(K, g, b, m, r)
    for grad in (dict(fly=fly), dict(dy=fly[1])):
        for xcoeff in (None, xc):
            def pair(need_dx=True):
                out = K.gemm_backward_small(w, x, xcoeff, need_dx=need_dx, **grad)
                assert out is not None, "shape not in the small regime"
                return out
            check(pair)
            check(lambda: pair(False))
            check(lambda: K.both(w, x, xcoeff, **grad))


@pytest.mark.parametrize("b,m,ns,kin,mout", [(3, 77, 64, 64, 128), (3, 200, 32, 128, 256), (1, 128, 16, 128, 256)])
def test_pool_gram_backward(b, m, ns, kin, mout, monkeypatch):
    # (the forward's decisions, as in test_gpu_mlp.py test_pooled_backward_from_the_gram_matrix: the
    # product takes the (256,128) path from 4096 chunks on; the backward checks coverage only)
    monkeypatch.setenv("MLP_POOL_GRAM256_MIN_CHUNKS", "64")
    monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "0")
    K = _K()
    g = _gen(b, m, ns, kin, mout)
    y2 = _randn(g, b, kin, m, ns, scale=1.3, shift=0.2)
    y2[:, :, :, 3] = y2[:, :, :, 1]
    w3 = (torch.randn(mout, kin, generator=g) / kin ** 0.5).to(DEV)
    g2, be2 = _bn_params(g, kin)
    g3, be3 = _bn_params(g, mout)
    c2 = K.bn_coefficients(y2, g2, be2, *_running(kin)(), 0.1, 1e-5, True)
    assert K.pool_gram_supported(w3, y2, ns)
    y3, mean3, invstd3, sc3, sh3, ext = K.gemm_forward_bn(w3, y2, (c2[2], c2[3]), g3, be3, *_running(mout)(),
                                                          0.1, 1e-5, pool=True)
    pooled, argmax, ymax = K.bn_relu_pool(y3, sc3, sh3) if ext is None else K.pool_from_extrema(ext, sc3, sh3)
    dpooled = _randn(g, b, mout, m)
    check(lambda: K.bn_relu_pool_backward_stats(None, dpooled, argmax, ymax, g3, sc3, sh3, mean3, invstd3, True, ns=ns))
    _, _, coef3 = K.bn_relu_pool_backward_stats(None, dpooled, argmax, ymax, g3, sc3, sh3, mean3, invstd3, True,
                                                ns=ns)
    check(lambda: K.pool_gram_backward(w3, y2, c2, g2, coef3, (mean3, invstd3, sc3, sh3), dpooled, argmax, ymax,
                                       ns, True))


def test_first_layer_of_four_channels():
    """wgrad_first4 (with and without the forward's moments), first4_moments, first4_bn at (2,33,4)"""
    K = _K()
    b, groups, ns = 2, 33, 4
    g = _gen(b, groups, ns)
    w = (torch.randn(64, 4, generator=g) * 0.5).to(DEV)
    x = _randn(g, b, 4, groups, ns, scale=2.0, shift=0.7)
    gamma, beta = _bn_params(g, 64)
    check(lambda: K.first4_moments(x))
    mom = K.first4_moments(x)
    check(lambda rm, rv: (K.first4_bn(mom, x.numel() // 4, w, gamma, beta, rm, rv, 0.1, 1e-5), rm, rv), _running(64))
    y = K.gemm_forward(w, x, None)
    mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, *_running(64)(), 0.1, 1e-5, True)
    dz = _randn(g, b, 64, groups, ns)
    _, _, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, True)
    fly = (y, dz, scale, shift, mean, invstd, coef)
    for moments in (None, mom):
        def run():
            dw = K.wgrad_first4(w, x, fly, moments)
            assert dw is not None
            return dw
        check(run)


@pytest.mark.parametrize("form", ["default", "tickets"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(2, 7, 33, 5), (1, 3, 7, 8), (4, 128, 64, 4), (8, 128, 256, 1), (3, 259, 250, 4)])
def test_batchnorm_relu_pool_kernels(shape, training, form, monkeypatch):
    """bn_coefficients, bn_relu_apply, bn_relu_pool, their backwards and both *_stats forms; the last
    two shapes are per-channel forms (one workgroup per channel) unless MLP_BN_CHANNEL_FORM=0 sends
    them to the ticket forms like the others"""
    if form == "tickets":
        monkeypatch.setenv("MLP_BN_CHANNEL_FORM", "0")
    K = _K()
    b, c, m, ns = shape
    g = _gen(*shape)
    y = _randn(g, *shape, scale=2.0, shift=0.5)
    gamma, beta = _bn_params(g, c)
    rm0, rv0 = _randn(g, c, scale=0.1), (torch.rand(c, generator=g) + 0.5).to(DEV)
    state = lambda: (rm0.clone(), rv0.clone())  # noqa: E731
    tk = K.new_tickets(c, DEV)  # one array through every launch: each must leave it zero
    check(lambda rm, rv: (K.bn_coefficients(y, gamma, beta, rm, rv, 0.1, 1e-5, training, tk), rm, rv, tk), state)
    mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, *state(), 0.1, 1e-5, training)
    check(lambda: K.bn_relu_apply(y, scale, shift))
    check(lambda: K.bn_relu_pool(y, scale, shift))
    dz, dpooled = _randn(g, *shape), _randn(g, b, c, m)
    check(lambda: (K.bn_relu_backward(y, dz, gamma, scale, shift, mean, invstd, training, tk), tk))
    check(lambda: (K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, training, tk), tk))
    _, argmax, ymax = K.bn_relu_pool(y, scale, shift)
    check(lambda: (K.bn_relu_pool_backward(y, dpooled, argmax, ymax, gamma, scale, shift, mean, invstd, training, tk),
                   tk))
    check(lambda: (K.bn_relu_pool_backward_stats(y, dpooled, argmax, ymax, gamma, scale, shift, mean, invstd,
                                                 training, tickets=tk), tk))
    assert int(tk.abs().max()) == 0


def test_pregather_kernels():
    K, E = _K(), _E()
    b, n, c, m, ns = 2, 1000, 64, 300, 8
    assert K.pregather_supported(b, c, n, m, ns)
    g = _gen(b, n, c, m, ns)
    xyz = (torch.rand(b, n, 3, generator=g) * 4 - 2).to(DEV)
    new_xyz = xyz[:, torch.randperm(n, generator=g)[:m].to(DEV)].contiguous()
    feats = _randn(g, b, c, n)
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(DEV)
    idx[:, :, 1] = idx[:, :, 0]
    check(lambda: K.pregather_pack(xyz, new_xyz, feats, 2.5))
    src = K.pregather_pack(xyz, new_xyz, feats, 2.5)
    w = (torch.randn(64, 3 + c, generator=g) / 8).to(DEV)
    z_ext = K.gemm_forward(w, src)
    gamma, beta = _bn_params(g, 64)
    check(lambda: K.pregather_forward(z_ext, idx, n))
    check(lambda rm, rv: (K.pregather_forward(z_ext, idx, n, (gamma, beta, rm, rv, 0.1, 1e-5)), rm, rv), _running(64),
          min_bytes=1)
    y, mean, invstd, scale, shift = K.pregather_forward(z_ext, idx, n, (gamma, beta, None, None, 0.1, 1e-5))
    dz = _randn(g, b, 64, m, ns)
    _, _, coef = K.bn_relu_backward_stats(y, dz, gamma, scale, shift, mean, invstd, True)
    check(lambda: E.group_inverse(idx, n), min_count=0)  # (an integer result: equality only)
    inverse = E.group_inverse(idx, n)
    assert inverse is not None
    check(lambda: K.pregather_backward((y, dz, scale, shift, mean, invstd, coef), inverse, n))
    dsrc = _randn(g, b, 3 + c, n + m)
    check(lambda: K.pregather_unpack_grad(dsrc, n, m))


def test_eval_pool_kernels():
    """one covered shape each: three clouds whose tiles share workgroups, a last workgroup with one tile"""
    import eval_pool_cases as C
    K = _K()
    wts = C.weights("lin4", 128, seed=1, device=DEV)
    x4 = C.input_lin4(3, 8, 32, seed=1, device=DEV)
    assert K.eval_lin4_supported(3, 4, 64, 128, 8, 32)
    (w0, w1, w2), (c0, c1, c2) = wts["w"], wts["coeff"]
    check(lambda: K.eval_lin4_pool(x4, K.eval_lin4_prepare(w0, c0, w1, w2), c1, c2), min_count=2, min_bytes=1)
    for c_out in (128, 256):
        wts = C.weights("stored", c_out, seed=2, device=DEV)
        y0 = C.input_stored(3, 3, 32, seed=2, device=DEV)
        assert K.eval_stored_supported(3, 128, 128, c_out, 3, 32)
        (w1, w2), (c0, c1, c2) = wts["w"], wts["coeff"]
        check(lambda: K.eval_stored_pool(y0, c0, K.eval_stored_prepare(w1, w2), c1, c2), min_count=2, min_bytes=1)


# ---- pointnet2._ext ----
def test_gather_points_and_grad():
    E = _E()
    b, c, n, m = 2, 5, 500, 77
    g = _gen(b, c, n, m)
    pts, gout = _randn(g, b, c, n), _randn(g, b, c, m)
    idx = torch.randint(0, n, (b, m), generator=g, dtype=torch.int32).to(DEV)
    idx[:, 5] = idx[:, 4]
    check(lambda: E.gather_points(pts, idx))
    check(lambda: E.gather_points_grad(gout, idx, n), atomic="gather_points_grad")


@pytest.mark.parametrize("b,n,m", [(3, 37, 5), (1, 2500, 2049)])
def test_three_nn_and_weights(b, n, m):
    E = _E()
    g = _gen(b, n, m)
    unknown, known = (torch.rand(b, n, 3, generator=g) * 2).to(DEV), (torch.rand(b, m, 3, generator=g) * 2).to(DEV)
    known[:, m // 2] = known[:, 0]
    dist2, _ = check(lambda: E.three_nn(unknown, known))
    check(lambda: E.three_nn_weights(dist2))


@pytest.mark.parametrize("b,c,m,n", [(2, 33, 50, 2052), (1, 5, 2049, 4096)])
def test_three_interpolate_family(b, c, m, n):
    E = _E()
    g = _gen(b, c, m, n)
    pts = _randn(g, b, c, m)
    idx = torch.randint(0, m, (b, n, 3), generator=g, dtype=torch.int32).to(DEV)
    idx[:, ::7, 1] = idx[:, ::7, 0]
    w = torch.rand(b, n, 3, generator=g)
    w = (w / w.sum(dim=2, keepdim=True)).to(DEV)
    gout = _randn(g, b, c, n)
    atomic = "three_interpolate_grad" if m > 1024 else None  # (m <= 1024: one LDS copy per wave, fixed order)
    check(lambda: E.three_interpolate(pts, idx, w))
    check(lambda: E.three_interpolate_grad(gout, idx, w, m), atomic=atomic)
    wide = _randn(g, b, c + 9, n)
    check(lambda: E.three_interpolate_grad_from(wide, 7, c, idx, w, m), atomic=atomic)
    # the two that write into the caller's tensor: allocated by the caller under the poison, so the
    # channels outside the written ranges must come back as the fill and the rest as the clean values
    rows = _randn(g, b, 4, n)
    for fill in FILLS:
        want = E.three_interpolate(pts, idx, w)
        with poisoned(fill) as p:
            out = torch.empty((b, c + 9, n), dtype=torch.float32, device=DEV)
            E.three_interpolate_into(pts, idx, w, out, 7)
            both = torch.empty((b, c + 9, n), dtype=torch.float32, device=DEV)
            E.three_interpolate_rows_into(pts, idx, w, both, 5, rows, 1)
        assert p.count == 2
        assert torch.equal(_bits(out[:, 7:7 + c]), _bits(want))
        assert torch.equal(_bits(both[:, 5:5 + c]), _bits(want)) and torch.equal(both[:, 1:5], rows)
        untouched = torch.full((), fill, device=DEV).expand(b, 1, n)
        for t, chans in ((out, list(range(7)) + [7 + c, 8 + c]), (both, [0] + list(range(5 + c, 9 + c)))):
            for ch in chans:
                assert torch.equal(_bits(t[:, ch:ch + 1]), _bits(untouched)), ch
    if E.three_interpolate_affine_supported(c, m, n):
        aw, ax = _randn(g, c, 3), _randn(g, b, 3, n)
        check(lambda: E.three_interpolate_affine(pts, idx, w, aw, ax))
    else:
        assert m > 2048


@pytest.mark.parametrize("c,n,m,ns", [(3, 500, 33, 7), (1, 40961, 33, 7)])
def test_group_points_family(c, n, m, ns):
    """(3,500,33,7): the LDS-privatised rows; (1,40961,33,7): a row that fits no LDS tier -- the output is
    zeroed by the library and added to with global atomics"""
    E = _E()
    b = 2
    g = _gen(c, n, m, ns)
    pts = _randn(g, b, c, n)
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(DEV)
    idx[:, :, ns // 2:] = idx[:, :, :1]
    gout = _randn(g, b, c, m, ns)
    check(lambda: E.group_points(pts, idx))
    check(lambda: E.group_points_grad(gout, idx, n), atomic="group_points_grad")
    inverse = E.group_inverse(idx, n)
    if inverse is not None:
        check(lambda: E.group_points_grad_sorted(gout, inverse, n))
    else:
        assert not E.group_inverse_supported(n, m, ns)


def test_query_and_group():
    """a 1000-point synthetic cloud: the group_concat path (idx given) and the brute-force query; the
    cell-list path on 4096 points, the smallest cloud that has cell lists (the lists themselves are
    integer workspaces: left alone)"""
    E = _E()
    load_pkg()
    synth = importlib.import_module("3dioumatch_amd.synth")
    b, m, r, ns, c = 2, 77, 0.3, 16, 5
    for n in (1000, 4096):
        xyz = torch.from_numpy(synth.cloud_uniform(b, n, synth.cube_side(n, r, ns), seed=n + m)).to(DEV)
        new_xyz = xyz[:, :m].contiguous()
        feats = _randn(_gen(n, m), b, c, n)
        assert E.grid_supported(b, n) == (n == 4096)
        for features in (feats, None):
            if n == 1000:
                idx = E.ball_query(new_xyz, xyz, r, ns)
                check(lambda: E.query_and_group(new_xyz, xyz, features, r, ns, True, idx=idx))
                check(lambda: E.query_and_group(new_xyz, xyz, features, r, ns, False))
            else:
                grid = E.build_grid(xyz, r)
                check(lambda: E.query_and_group(new_xyz, xyz, features, r, ns, True, grid=grid))


# ---- IoU ----
def test_iou_bindings():
    load_pkg()
    ut = importlib.import_module("pcdet.ops.iou3d_nms.iou3d_nms_utils")
    ed = importlib.import_module("3dioumatch_amd.votenet.eval_det")
    eh = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
    synth = importlib.import_module("3dioumatch_amd.synth")
    s, p, q = 3, 33, 7
    pairs = [synth.boxes_pair(p, seed=10 + i) for i in range(s)]
    a = torch.from_numpy(np.stack([x[0] for x in pairs])).to(DEV)          # (3,33,7)
    bb = torch.from_numpy(np.stack([x[1][:q] for x in pairs])).to(DEV)     # (3,7,7)
    for scene in range(s):
        check(lambda: ut.boxes_iou_bev(a[scene], bb[scene]))
        check(lambda: ut.boxes_iou3d_gpu(a[scene], bb[scene]))
    check(lambda: ut.boxes_iou3d_scene_max_gpu(a, bb))
    ca = eh.corners_upright_camera(a[:1, :, :3], a[:1, :, 3:6].double(), a[:1, :, 6].double())[0].contiguous()
    cb = eh.corners_upright_camera(bb[:1, :, :3], bb[:1, :, 3:6].double(), bb[:1, :, 6].double())[0].contiguous()
    check(lambda: ed.corners_iou3d_gpu(ca, cb))


# ===================================== tier 2: modules and steps =====================================
# The same three fills around a whole module call (forward and backward) or a whole step.  Modules
# built of the kernels above add nothing the hardware orders: poisoned == clean bit for bit, the
# project's own rule for the same computation run twice (tests/test_determinism.py,
# test_bwd_x6_roles.py).  The two train steps are held to test_train_step.py
# test_graph_replay_matches_eager's compare(): the bounds for eager against eager.
def _module_state(module):
    return [p.grad for p in module.parameters()] + [b for _, b in module.named_buffers()]


def test_shared_mlp_forward_pooled_with_backward():
    import copy
    load_pkg()
    P = importlib.import_module("pointnet2.pytorch_utils")
    torch.manual_seed(0)
    proto = P.SharedMLP([6, 16, 16, 32], bn=True).to(DEV).train()
    g = _gen(3, 6, 50, 16)
    x0, wgt = _randn(g, 3, 6, 50, 16), _randn(g, 3, 32, 50)

    def run(mlp):
        x = x0.clone().requires_grad_(True)
        out = mlp.forward_pooled(x)
        (out * wgt).sum().backward()
        return out, x.grad, _module_state(mlp)
    check(run, lambda: (copy.deepcopy(proto),))


def test_shared_mlp_forward_pregathered_with_backward():
    import copy
    load_pkg()
    P = importlib.import_module("pointnet2.pytorch_utils")
    E = _E()
    b, n, c, m, ns, scale = 2, 1000, 64, 300, 8, 2.5
    g = _gen(b, n, c, m, ns, 1)
    xyz = (torch.rand(b, n, 3, generator=g) * 4 - 2).to(DEV)
    new_xyz = xyz[:, torch.randperm(n, generator=g)[:m].to(DEV)].contiguous()
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(DEV)
    idx[:, :, 1] = idx[:, :, 0]
    inverse = E.group_inverse(idx, n)
    feats0 = _randn(g, b, c, n)
    torch.manual_seed(5)
    proto = P.SharedMLP([c + 3, 64, 128], bn=True).to(DEV).train()
    assert proto.pregather_ok(xyz, new_xyz, feats0, m, ns)
    dout = _randn(g, b, 128, m)

    def run(mlp):
        feats = feats0.clone().requires_grad_(True)
        out = mlp.forward_pregathered(xyz, new_xyz, feats, idx, inverse, scale)
        out.backward(dout)
        return out, feats.grad, _module_state(mlp)
    check(run, lambda: (copy.deepcopy(proto),))


def test_fused_head_chain_with_backward():
    import copy
    load_pkg()
    fh = importlib.import_module("3dioumatch_amd.votenet.fused_head")
    nn = torch.nn
    cin, mid, cout, (b, r) = 128, 128, 79, (3, 256)
    torch.manual_seed(cin + cout)
    proto = [nn.Conv1d(cin, mid, 1), nn.BatchNorm1d(mid), nn.Conv1d(mid, mid, 1), nn.BatchNorm1d(mid),
             nn.Conv1d(mid, cout, 1)]
    for mod in proto:
        if isinstance(mod, nn.BatchNorm1d):
            mod.weight.data.uniform_(0.5, 1.5); mod.bias.data.normal_(0, 0.3)
            mod.running_mean.normal_(0, 0.2); mod.running_var.uniform_(0.5, 1.5)
    proto = [mod.to(DEV).train() for mod in proto]
    g = _gen(cin, mid, cout, b, r)
    x0, gout = _randn(g, b, cin, r), _randn(g, b, cout, r)

    def run(*mods):
        x = x0.clone().requires_grad_(True)
        out = fh.head_chain(x, *mods)
        out.backward(gout)
        return out, x.grad, [_module_state(mod) for mod in mods]
    check(run, lambda: tuple(copy.deepcopy(mod) for mod in proto))


def test_vote_tail_and_unit_length_features_with_backward():
    load_pkg()
    heads = importlib.import_module("3dioumatch_amd.votenet.heads")
    D = importlib.import_module("3dioumatch_amd.votenet.detector")
    b, c, n = 2, 37, 100
    g = _gen(b, c, n)
    leaves = [_randn(g, b, 3 + c, n), _randn(g, b, n, 3), _randn(g, b, c, n)]
    g_xyz, g_feat = _randn(g, b, n, 3), _randn(g, b, c, n)

    def tail():
        net, xyz, feats = (t.clone().requires_grad_(True) for t in leaves)
        assert heads.vote_tail_fused(xyz, feats)
        vote_xyz, vote_feats, norm = heads.vote_tail(net, xyz, feats)
        torch.autograd.backward([vote_xyz, vote_feats], [g_xyz, g_feat])
        return vote_xyz, vote_feats, norm, net.grad, xyz.grad, feats.grad
    check(tail)
    x0, wgt = _randn(g, 2, 7, 100, scale=3.0), _randn(g, 2, 7, 100)

    def unit():
        x = x0.clone().requires_grad_(True)
        y = D.unit_length_features(x)
        (y * wgt).sum().backward()
        return y, x.grad
    check(unit)


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_fused_supervised_loss_with_backward(tag, oracle_omp, monkeypatch):
    """the inputs of tests/test_fused_loss.py: the seeded network's forward on the seeded batch (outside
    the poison), its outputs as leaves; the loss pass and its backward under the poison"""
    import test_fused_loss as T
    V, dev = T._setup(True, oracle_omp)
    fused = importlib.import_module("3dioumatch_amd.votenet.fused_loss")
    monkeypatch.setenv("VOTENET_FUSED_LOSS", "1")
    assert fused.enabled()
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    _, forward = T._forward(V, cfg, dev)
    ep0 = forward()
    ep0["all_supervised"] = True
    keys = sorted(k for k, v in ep0.items() if torch.is_tensor(v) and v.requires_grad)
    assert keys

    def run():
        ep = {k: (v.detach().clone().requires_grad_(v.requires_grad) if torch.is_tensor(v) else v)
              for k, v in ep0.items()}
        leaves = [ep[k] for k in keys]
        loss, out = V.get_labeled_loss(ep, cfg, {"dataset_config": cfg})
        loss.backward()
        return (loss.detach(), [out[k].detach() for k in T.LABELS + ("pred_bbox",)],
                [out[k].detach() for k in T.LOGGED if k in out], [t.grad for t in leaves])
    check(run)


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_fused_consistency_loss_with_backward(tag, oracle_omp, monkeypatch):
    """tests/golden/unlabeled_loss_ref.npz: the reference's inputs of the consistency loss"""
    import test_fused_loss as T
    from conftest import golden
    T._setup(True, oracle_omp)
    V = importlib.import_module("3dioumatch_amd.votenet")
    U = importlib.import_module("3dioumatch_amd.votenet.losses_unlabeled")
    monkeypatch.setenv("VOTENET_FUSED_LOSS", "1")
    g = golden("unlabeled_loss_ref.npz")
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    keys = ("center", "heading_residuals_normalized", "size_residuals_normalized", "sem_cls_scores",
            "heading_scores", "size_scores", "objectness_scores")
    ep0 = {k.split("::", 1)[1]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith(tag + "_in_ep::")}
    ema = {k.split("::", 1)[1]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith(tag + "_in_ema::")}
    labeled = int(ep0["supervised_mask"].sum())

    def run():
        ep = {k: v.clone() for k, v in ep0.items()}
        for k in keys:
            ep[k].requires_grad_(True)
        leaves = [ep[k] for k in keys]
        ep["labeled_num"] = labeled
        loss, out = U.get_unlabeled_loss(ep, ema, cfg, U.default_config_dict(cfg, dataset=tag, unlabeled_batch_size=3))
        loss.backward()
        produced = sorted(k for k, v in out.items() if k.startswith("unlabeled_") and torch.is_tensor(v))
        return loss.detach(), [out[k].detach() for k in produced], [t.grad for t in leaves]
    check(run)


@pytest.mark.parametrize("tag,s,k,empty", [("scannet", 3, 64, False), ("sunrgbd", 5, 256, False),
                                           ("scannet", 3, 64, True)])
def test_pseudo_labels_with_view_stats(tag, s, k, empty, monkeypatch):
    """pseudo_labels_gpu + lhs_pseudo_stats through get_unlabeled_loss(view_stats=True); empty: no
    teacher proposal passes the objectness threshold (confident = 0.0) -- every slot empty, every
    label a default the kernels write themselves"""
    from test_view_stats import STAT_KEYS, run_loss
    from test_view_stats_gpu import _random_case
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    U = importlib.import_module("3dioumatch_amd.votenet.losses_unlabeled")
    monkeypatch.setenv("VOTENET_FUSED_PSEUDO_LABELS", "1")
    cfg0 = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    cfg, ep, ema = _random_case(V, tag, s, k, cfg0.num_class, seed=s * 7 + k)
    if empty:
        ema["objectness_scores"][..., 1] = ema["objectness_scores"][..., 0] - 5.0

    def run():
        loss, out = run_loss(U, cfg, tag, ep, ema, True)
        assert (int(out["unlabeled_box_label_mask"].sum()) == 0) == empty
        produced = sorted(key for key, v in out.items() if key.startswith("unlabeled_") and torch.is_tensor(v))
        # all twelve slots of lhs_pseudo_stats' `stats`, whatever their names
        return (loss.detach(), [out[key].detach() for key in produced], [out[key].detach() for key in STAT_KEYS],
                out["pseudo_gt_ratio"])
    check(run)


def test_iou_opt_wrapper():
    """votenet/iou_opt.py's own allocations (`whole`, `rel` of HipBoxStep.forward, `grad` of gradient):
    two refinement steps of optimize_boxes(engine="hip") and one gradient on a small synthetic batch;
    the detector's forward runs outside the poison"""
    from test_iou_opt_gpu import _scene
    load_pkg()
    O = importlib.import_module("3dioumatch_amd.votenet.iou_opt")
    det, ep, _ = _scene("scannet", b=2, n=20000)
    center, size = ep["center"].detach(), ep["size"].detach()

    def run():
        out = O.optimize_boxes(det, ep, 1e-3, 2, engine="hip")
        hc, hs = O.HipBoxStep(det, ep).gradient(center, size)
        return out["center"], out["size_residuals"], out["iou_scores"], hc, hs
    clean = check(run, min_count=3)
    assert float((clean[0] - center).abs().max()) > 0  # the boxes moved


def test_iou_opt_box_step():
    """votenet_iou_opt_box_step at (3,13,300,64), as tests/test_iou_opt_gpu.py calls it; the gradient
    tensor is the caller's allocation"""
    load_pkg()
    L = importlib.import_module("3dioumatch_amd._lib")
    from test_iou_opt_gpu import _unit
    b, k, nseed, ch, m, rate = 3, 13, 300, 64, 128, 0.25
    g = _gen(b, k, nseed, ch)
    room = torch.tensor([6.0, 5.0, 3.0])
    seed_xyz = (torch.rand(b, nseed, 3, generator=g) * room).to(DEV)
    center = (torch.rand(b, k, 3, generator=g) * room).to(DEV)
    size = (torch.rand(b, k, 3, generator=g) * 0.6 + 0.05).to(DEV)
    heading = ((torch.rand(b, k, generator=g) - 0.5) * 6.0).to(DEV)
    idx = torch.randint(0, nseed, (b, k * 64, 3), generator=g, dtype=torch.int32).to(DEV)
    w0 = _randn(g, m, 3 + ch, scale=0.1)
    proj = torch.matmul(w0[:, 3:], _randn(g, b, ch, nseed)).contiguous()
    dy0 = _randn(g, b, m, k * 64, scale=1e-3)
    unit = _unit(torch.device(DEV))

    def run(c1, s1):
        grad = torch.empty(b, k, 6, device=DEV)
        with torch.cuda.device(torch.device(DEV)):
            L.check(L.lib.votenet_iou_opt_box_step(
                b, k, nseed, m, unit.data_ptr(), seed_xyz.data_ptr(), idx.data_ptr(), proj.data_ptr(),
                w0.data_ptr(), w0.shape[1], dy0.data_ptr(), None, None, None, None, heading.data_ptr(), rate,
                c1.data_ptr(), s1.data_ptr(), grad.data_ptr(), torch.cuda.current_stream().cuda_stream),
                "votenet_iou_opt_box_step")
        return c1, s1, grad
    check(run, lambda: (center.clone(), size.clone()))


def _step_compare(eager, other, tag):
    """tests/test_train_step.py test_graph_replay_matches_eager compare(): eager against eager up to the
    order of the fp32 atomics"""
    assert torch.equal(eager["inds"], other["inds"]), tag
    assert abs(eager["loss"] - other["loss"]) <= 1e-5 * max(1.0, abs(eager["loss"])), tag
    g = float((eager["grad"] - other["grad"]).norm() / eager["grad"].norm())
    p = float((eager["params"] - other["params"]).abs().max())
    print("poisoned vs clean, %s: gradient rel %.2e, parameters max abs %.2e" % (tag, g, p))
    assert g < 1e-5, (tag, g)
    assert p <= 2e-4, (tag, p)
    assert float((eager["params"] - other["params"]).norm() / eager["params"].norm()) < 1e-4, tag
    for (n_e, b_e), (_, b_g) in zip(eager["buffers"], other["buffers"]):
        if n_e.endswith("running_mean") or n_e.endswith("running_var"):
            assert torch.allclose(b_e, b_g, rtol=1e-4, atol=2e-6), (tag, n_e)
        elif n_e.endswith("num_batches_tracked"):
            assert int(b_e) == int(b_g), (tag, n_e)


def _one_step(make_runner, batch, extra=()):
    """one eager step from the seeded weights under each fill (None: clean)"""
    step_mod = importlib.import_module("3dioumatch_amd.votenet.step")
    results = []
    for fill in (None,) + FILLS:
        runner = make_runner()
        assert not runner.graphs
        step_mod.freeze_shift_invariant_parameters(runner.net)
        torch.manual_seed(9)
        torch.cuda.manual_seed_all(9)
        view = dict(batch)
        if fill is None:
            loss, ep = runner(view)
        else:
            with poisoned(fill) as p:
                loss, ep = runner(view)
            assert p.count > 0
        torch.cuda.synchronize()
        out = {"loss": float(loss.detach()), "inds": ep["aggregated_vote_inds"].cpu().clone(),
               "grad": step_mod.flat_grads(runner.net).cpu().clone(),
               "params": step_mod.flat_params(runner.net).cpu().clone(),
               "buffers": [(n, b.detach().cpu().clone()) for n, b in runner.net.named_buffers()],
               "extra": [ep[k].detach().cpu().clone() for k in extra]}
        assert math.isfinite(out["loss"])
        for t in [out["grad"], out["params"]] + [b for _, b in out["buffers"]] + out["extra"]:
            assert bool(torch.isfinite(t.double()).all())
        results.append(out)
    for name, got in zip(FILL_IDS, results[1:]):
        _step_compare(results[0], got, name)
        for a, c in zip(results[0]["extra"], got["extra"]):
            assert torch.equal(a, c), name
    return results


def test_supervised_step():
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    data = importlib.import_module("3dioumatch_amd.votenet.data")
    cfg = V.scannet_config()
    dev = torch.device(DEV)
    batch = data.make_batch(2, 20000, cfg, seed=44, num_objects=5, device=dev)
    _one_step(lambda: V.SupervisedStep(cfg, dev, world_size=1, num_proposal=64, seed=3, graphs=False), batch)


def test_semi_supervised_step():
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    U = importlib.import_module("3dioumatch_amd.votenet.losses_unlabeled")
    cfg = V.scannet_config()
    dev = torch.device(DEV)
    batch = {k: v.to(dev) for k, v in V.make_semi_batch(2, 3, 20000, cfg, seed=5, num_objects=5).items()}

    def make_runner():
        cd = U.default_config_dict(cfg, unlabeled_batch_size=3)
        cd.update(obj_threshold=0.3, cls_threshold=0.03, iou_threshold=0.2)  # random weights: loosen
        return V.SemiSupervisedStep(cfg, dev, num_proposal=64, seed=4, graphs=False, config_dict=cd)
    results = _one_step(make_runner, batch, extra=("unlabeled_box_label_mask",))
    assert int(results[0]["extra"][0].sum()) > 0


def test_inference_engine_evaluate():
    """one evaluate pass (host parsers, then the device parsers with the loss meter) on a small synthetic
    batch, the engine -- its weight images and folded coefficients -- built under the poison too: the
    metrics equal the clean pass's, NaN matching NaN (a class without ground truth)"""
    from test_inference_gpu import _detector, _mods
    _, V, I, step, data = _mods()
    det, cfg = _detector(V, step, "scannet")
    config_dict = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
                   "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
                   "per_class_proposal": True, "conf_thresh": 0.05}
    batches = [data.make_batch(2, 20000, cfg, seed=40, device=torch.device(DEV))]

    def run():
        engine = I.InferenceEngine(det, graphs=False)
        host = I.evaluate(engine, batches, config_dict, opt_step=0)
        device, stats = I.evaluate(engine, batches, config_dict, device_ap=True, with_loss=True)
        return host, device, stats

    def same(a, b):
        assert set(a) == set(b)
        for key, val in b.items():
            assert a[key] == val or (math.isnan(a[key]) and math.isnan(val)), (key, a[key], val)

    clean = run()
    for fill, name in zip(FILLS, FILL_IDS):
        with poisoned(fill) as p:
            got = run()
        assert p.count > 0, name
        for ga, ca in zip(got[:2], clean[:2]):
            assert len(ga) == len(ca)
            for g_, c_ in zip(ga, ca):
                same(g_, c_)
        same(got[2], clean[2])
        assert all(math.isfinite(v) for v in got[2].values()), name
