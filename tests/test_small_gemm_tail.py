"""The small layers' GEMM kernels (csrc/mlp_gemm.hip: gemm_nn_small_body, wgrad_direct_body) at the
shapes where their epilogue can go wrong.  After the reduction loop every one of a workgroup's four
waves finishes and stores ONE 32 x 32 tile of the 64 x 64 output tile (tile_owner_sum), so a shape
decides which owners store whole tiles, single rows or nothing at all:

  (1, 64, 64, 64)        the full tile
  (2, 79, 128, 100)      ragged rows in the second row block, an owner with no row, columns not a
                         multiple of 64; the bias row
  (3, 33, 70, 37)        odd r (scalar loads), K not a multiple of 16, an owner with exactly one row
  (1, 20, 259, 8)        both i = 1 owners and both j = 1 owners store nothing
  (8, 128, 128, 256), (8, 256, 256, 1024)   the train step's head and FP shapes
  (8, 256, 256, 2048)    the column limit of the small regime, several weight-gradient slices

Every shape runs the forward (plain and BatchNorm + ReLU'ed input, weight as fp32 and as bf16 image,
bias on the m = 79 shape), the transposed form (gradient operand given, formed on the fly, and formed
from a pooled layer's arg-max), the pair launch and the direct weight gradient.

Truth: float64 torch on the fp32 inputs.  Bound: the rule tests/test_gpu_mlp.py applies to these
entry points (`close`: max |got - want| <= tol * max(1, max |want|), tol 2e-5 forward, 3e-5 data
gradient, 1e-4 weight gradient).  Every call also runs with its outputs and workspaces inside
NaN-pattern guards on NaN-filled memory (guards intact, every output element written) and twice
(bit-equal results)."""
import contextlib
import functools
import importlib

import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 64, 64, 64), (2, 79, 128, 100), (3, 33, 70, 37), (1, 20, 259, 8), (8, 128, 128, 256),
          (8, 256, 256, 1024), (8, 256, 256, 2048)]
TOL_FWD, TOL_DGRAD, TOL_WGRAD = 2e-5, 3e-5, 1e-4   # tests/test_gpu_mlp.py, the same entry points

GUARD = 64             # floats on either side of every allocation (keeps 256-byte alignment)
PATTERN = 0x7FC0DEAD   # a quiet NaN with a payload nothing computes


class Guarded(object):
    """torch.empty / torch.empty_like of the bindings hand out the middle of a larger buffer that is
    filled with PATTERN, guards and interior alike."""

    def __init__(self):
        self.buffers = []

    def wrap(self, t):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.numel() == 0:
            return t
        n = t.numel()
        big = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=t.device)
        self.buffers.append((big, n))
        return big[GUARD:GUARD + n].view(torch.float32).view(t.shape)

    def check(self):
        assert self.buffers, "nothing was allocated inside the block"
        for big, n in self.buffers:
            assert bool((big[:GUARD] == PATTERN).all()), "guard in front of an allocation overwritten"
            assert bool((big[GUARD + n:] == PATTERN).all()), "guard behind an allocation overwritten"


@contextlib.contextmanager
def guarded():
    rec = Guarded()
    real_empty, real_empty_like = torch.empty, torch.empty_like
    torch.empty = lambda *a, **k: rec.wrap(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: rec.wrap(real_empty_like(*a, **k))
    try:
        yield rec
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like


def _k():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


def close64(got, want, tol, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what + ": an element was not written"
    err = float((got.double() - want).abs().max())
    scale = max(1.0, float(want.abs().max()))
    print("%s: max error %.3g, bound %.3g" % (what, err, tol * scale))
    assert err <= tol * scale, (what, err, tol * scale)


def run(fn, what):
    """fn() inside the guards, then once more: -> tuple of result tensors (None entries kept)"""
    with guarded() as rec:
        first = fn()
    torch.cuda.synchronize()
    rec.check()
    second = fn()
    first = first if isinstance(first, tuple) else (first,)
    second = second if isinstance(second, tuple) else (second,)
    for a, b in zip(first, second):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b), what + ": a second call differs"
    return first


def pool_ns(r):
    """samples per pooling group for r columns: 16 (a 16-column segment inside one group) where r
    allows it, else 4, else the whole row as one group"""
    return 16 if r % 16 == 0 else (4 if r % 4 == 0 else r)


@functools.lru_cache(maxsize=None)
def case(shape):
    """the inputs of one shape on the device and the float64 results, computed once"""
    b, m, k, r = shape
    g = torch.Generator().manual_seed(b * 100003 + m * 1009 + k * 31 + r)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    c = {}
    c["w"] = (rn(m, k) / k ** 0.5).to(DEV)
    c["x"] = rn(b, k, r).to(DEV)
    c["bias"] = rn(m).to(DEV)
    c["xc"] = ((ru(k) + 0.5).to(DEV), (rn(k) * 0.3).to(DEV))
    c["y"] = rn(b, m, r).to(DEV)
    c["dz"] = rn(b, m, r).to(DEV)
    sc, sh = (ru(m) + 0.5).to(DEV), (rn(m) * 0.3).to(DEV)
    mu, istd = (rn(m) * 0.2).to(DEV), (ru(m) + 0.5).to(DEV)
    coef = torch.stack([ru(m) + 0.5, rn(m) * 0.1, rn(m) * 0.1], dim=1).contiguous().to(DEV)
    c["fly"] = (c["y"], c["dz"], sc, sh, mu, istd, coef)
    ns = pool_ns(r)
    groups = r // ns
    dpooled = rn(b, m, groups).to(DEV)
    argmax = torch.randint(0, ns, (b, m, groups), generator=g, dtype=torch.int32).to(DEV)
    c["pooled"] = (c["y"].view(b, m, groups, ns), dpooled, argmax, sc, sh, mu, istd, coef)

    d = lambda t: t.double()  # noqa: E731
    bc = lambda v: d(v)[None, :, None]  # noqa: E731
    w64, x64, y64 = d(c["w"]), d(c["x"]), d(c["y"])
    xz64 = torch.relu(x64 * bc(c["xc"][0]) + bc(c["xc"][1]))
    gate = (y64 * bc(sc) + bc(sh) > 0).double()
    lin = bc(coef[:, 1]) + (y64 - bc(mu)) * bc(istd) * bc(coef[:, 2])
    dy_fly = bc(coef[:, 0]) * (d(c["dz"]) * gate - lin)
    won = torch.zeros(b, m, groups, ns, dtype=torch.float64, device=DEV)
    won.scatter_(3, argmax.long()[..., None], d(dpooled)[..., None])
    dy_pool = bc(coef[:, 0]) * (won.view(b, m, r) * gate - lin)
    c["t_fwd"] = {False: torch.matmul(w64, x64), True: torch.matmul(w64, xz64)}
    c["t_dx"] = {"dy": torch.matmul(w64.t(), d(c["dz"])), "fly": torch.matmul(w64.t(), dy_fly),
                 "pooled": torch.matmul(w64.t(), dy_pool)}
    c["t_dw"] = {(gk, bn): torch.einsum("bmr,bkr->mk", gv, xv)
                 for gk, gv in (("dy", d(c["dz"])), ("fly", dy_fly))
                 for bn, xv in ((False, x64), (True, xz64))}
    c["images"] = _k().WeightImages([c["w"]])
    c["images"].refresh()
    return c


def _grad(c, kind):
    return {"dy": dict(dy=c["dz"]), "fly": dict(fly=c["fly"]), "pooled": dict(pooled=c["pooled"])}[kind]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward(shape):
    """gemm_nn_small_kernel / gemm_nn_small_bias_kernel, OP_DIRECT and OP_BNRELU, with and without
    the weight image; with the bias on the m = 79 shape"""
    K, c = _k(), case(shape)
    b, m, k, r = shape
    assert K._lib.mlp_gemm_image_supported(b, r), "not the small kernel"
    for bn in (False, True):
        coeff = c["xc"] if bn else None
        for image in (False, True):
            for bias in ((None, c["bias"]) if m == 79 else (None,)):
                what = "forward %s bn=%d image=%d bias=%d" % (shape, bn, image, bias is not None)
                with K.weight_images(c["images"] if image else None):
                    assert (K._image_of(c["w"], b, r) is not None) == image
                    (y,) = run(lambda: K.gemm_forward(c["w"], c["x"], coeff, bias), what)
                want = c["t_fwd"][bn] + (bias.double()[None, :, None] if bias is not None else 0.0)
                close64(y, want, TOL_FWD, what)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transposed(shape):
    """gemm_nn_small_kernel<., A_TRANS> through mlp_gemm_dgrad: OP_DIRECT, OP_DY, OP_POOLDY"""
    K, c = _k(), case(shape)
    for kind in ("dy", "fly", "pooled"):
        what = "dgrad %s %s" % (shape, kind)
        (dx,) = run(lambda: K.gemm_dgrad(c["w"], **_grad(c, kind)).view_as(c["x"]), what)
        close64(dx, c["t_dx"][kind], TOL_DGRAD, what)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair(shape):
    """gemm_small_backward_pair_kernel: both roles, every operand form, with and without the
    transposed weight image (read when the gradient operand is given) and without the data gradient.
    The direct weight gradient needs 32 columns: below that the entry declines."""
    K, c = _k(), case(shape)
    b, m, k, r = shape
    if r < 32:
        assert K.gemm_backward_small(c["w"], c["x"], None, dy=c["dz"]) is None
        return
    for kind in ("dy", "fly"):
        for bn in (False, True):
            for image in ((False, True) if kind == "dy" else (False,)):
                what = "pair %s %s bn=%d image=%d" % (shape, kind, bn, image)
                xcoeff = c["xc"] if bn else None
                with K.weight_images(c["images"] if image else None):
                    dx, dw = run(lambda: K.gemm_backward_small(c["w"], c["x"], xcoeff, **_grad(c, kind)), what)
                close64(dx, c["t_dx"][kind], TOL_DGRAD, what + " dx")
                close64(dw, c["t_dw"][(kind, bn)], TOL_WGRAD, what + " dw")
            none, dw_only = run(lambda: K.gemm_backward_small(c["w"], c["x"], xcoeff, need_dx=False,
                                                              **_grad(c, kind)), what + " dw alone")
            assert none is None
            assert torch.equal(dw_only, dw)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_gradient(shape):
    """gemm_wgrad_direct_kernel through mlp_gemm_wgrad, every operand form (r < 32: the staged kernel
    takes the layer -- checked against the same truth)"""
    K, c = _k(), case(shape)
    b, m, k, r = shape
    for kind in ("dy", "fly"):
        for bn in (False, True):
            what = "wgrad %s %s bn=%d" % (shape, kind, bn)
            (dw,) = run(lambda: K.gemm_wgrad(m, k, c["x"], c["xc"] if bn else None, **_grad(c, kind)), what)
            close64(dw, c["t_dw"][(kind, bn)], TOL_WGRAD, what)
