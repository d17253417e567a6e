"""The one-pass eval MLP kernels (csrc/mlp_eval_pool.hip) on the MI355X, called directly: all six
eval_stored_kernel<NS, M2B> and all three eval_lin4_kernel<NS> instantiations at the shapes of
tests/eval_pool_cases.py (less than a workgroup, a workgroup over two clouds, a one-tile tail, two
tiles per wave with a tail, aligned), held to

  * fp32-grade error: e(kernel) <= RATIO * e(plain fp32 torch), both against float64 on the same data,
    no absolute floor;
  * exact zeros where the float64 group maximum is safely negative; finite; every element written;
  * bit-exact invariances (torch.equal): a column's result depends only on that column, a group's only
    on the SET of its samples, so a permutation inside the groups, a roll of the groups, the number of
    clouds in the launch, the tiles-per-wave choice and a repeat launch change no bit;
  * rejections that launch nothing.

Each test prints its e(kernel) / e(plain) (pytest -s shows them; DESIGN.md has the table)."""
import functools
import importlib

import pytest
import torch

import eval_pool_cases as C
from conftest import load_pkg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ODD_ROLL = 5


@functools.lru_cache(maxsize=None)
def _K():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


@functools.lru_cache(maxsize=None)
def _stored_setup(c_out):
    wts = C.weights("stored", c_out, seed=0, device=DEV)
    return wts, _K().eval_stored_prepare(*wts["w"])


@functools.lru_cache(maxsize=None)
def _lin4_setup():
    wts = C.weights("lin4", 128, seed=0, device=DEV)
    w0, w1, w2 = wts["w"]
    return wts, _K().eval_lin4_prepare(w0, wts["coeff"][0], w1, w2)


def _stored(y0, c_out):
    wts, img = _stored_setup(c_out)
    c0, c1, c2 = wts["coeff"]
    return _K().eval_stored_pool(y0, c0, img, c1, c2)


def _lin4(x4):
    wts, img = _lin4_setup()
    return _K().eval_lin4_pool(x4, img, wts["coeff"][1], wts["coeff"][2])


def _abi_stored(y0_ptr, img_ptr, out, b, c_out, m, ns):
    """mlp_eval_stored_pool through the C ABI into a buffer of the caller's -> its return code"""
    K = _K()
    (s0, h0), (s1, h1), (s2, h2) = _stored_setup(256 if c_out == 192 else c_out)[0]["coeff"]
    with torch.cuda.device(DEV):
        return K._lib.mlp_eval_stored_pool(b, c_out, m, ns, y0_ptr, s0.data_ptr(), h0.data_ptr(), img_ptr,
                                           s1.data_ptr(), h1.data_ptr(), s2.data_ptr(), h2.data_ptr(),
                                           out.data_ptr(), K._stream(out))


def _abi_lin4(x4_ptr, img_ptr, out, b, m, ns):
    K = _K()
    _, (s1, h1), (s2, h2) = _lin4_setup()[0]["coeff"]
    with torch.cuda.device(DEV):
        return K._lib.mlp_eval_lin4_pool(b, m, ns, x4_ptr, img_ptr, s1.data_ptr(), h1.data_ptr(),
                                         s2.data_ptr(), h2.data_ptr(), out.data_ptr(), K._stream(out))


def _poisoned(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _check_values(tag, out, truth, pre, plain):
    e_k, e_p = C.rel_err(out, truth), C.rel_err(plain, truth)
    print("%s: e(kernel) %.3e  e(plain_fp32) %.3e  ratio %.2f" % (tag, e_k, e_p, e_k / e_p))
    assert torch.isfinite(out).all()
    assert e_k <= C.RATIO * e_p, (e_k, e_p)
    sure = pre < -(C.RATIO * e_p * truth.abs().max().item())
    assert sure.any()
    assert (out[sure] == 0).all()
    return e_k, e_p


def _check_invariances(run, x, out):
    """run: (b, c, m, ns) -> (b, c_out, m); out = run(x)"""
    b, _, m, ns = x.shape
    assert torch.equal(run(x), out)                                   # a repeat launch
    g = torch.Generator(device=DEV).manual_seed(11)
    perm = torch.rand(b, 1, m, ns, device=DEV, generator=g).argsort(3).expand_as(x)
    assert torch.equal(run(x.gather(3, perm).contiguous()), out)       # samples permuted inside the groups
    for k in (1, ODD_ROLL):
        assert torch.equal(run(x.roll(k, 2).contiguous()), out.roll(k, 2)), k   # groups rolled
    if b > 1:
        for i in range(b):                                             # each cloud launched alone
            assert torch.equal(run(x[i:i + 1].contiguous())[0], out[i]), i


@pytest.mark.parametrize("c_out", [128, 256])
@pytest.mark.parametrize("shape", C.STORED_SHAPES, ids=lambda s: "%s-ns%d" % (s[0], s[1]))
def test_stored_kernel(shape, c_out):
    K = _K()
    case, ns, b, m, tpw, tpc, total, _, _ = shape
    if case == "c":
        tpc = C.find_c_tiles(K.eval_stored_tiles_per_wave, c_out, ns, b)
        m = C.m_of_tiles(tpc, ns)
        total = C.tile_arith(b, m, ns, 2)[1]
        assert tpc % 2 == 1 and total % 8 != 0
        assert K.eval_stored_tiles_per_wave(1, c_out, m, ns) == 1     # the same clouds, launched alone
    assert K.eval_stored_supported(b, 128, 128, c_out, m, ns)
    assert K.eval_stored_tiles_per_wave(b, c_out, m, ns) == tpw
    if case in C.TAIL_CASES:
        assert total % (4 * tpw) != 0
    wts, img = _stored_setup(c_out)
    y0 = C.input_stored(b, m, ns, seed=ns, device=DEV)
    out = _stored(y0, c_out)
    assert out.shape == (b, c_out, m)
    truth, pre = C.truth_stored(y0, wts)
    _check_values("stored<%d,%d> %s (b %d, m %d, %d tiles per cloud, %d per wave)" % (ns, c_out // 32, case, b, m, tpc, tpw),
                  out, truth, pre, C.plain_fp32("stored", y0, wts))
    del truth, pre
    # the whole output is written: a launch into a poisoned buffer leaves no poison (and the same bits)
    buf = _poisoned(b, c_out, m)
    assert _abi_stored(y0.data_ptr(), img.data_ptr(), buf, b, c_out, m, ns) == 0
    assert torch.equal(buf, out)
    _check_invariances(lambda x: _stored(x, c_out), y0, out)


@pytest.mark.parametrize("shape", C.LIN4_SHAPES, ids=lambda s: "%s-ns%d" % (s[0], s[1]))
def test_lin4_kernel(shape):
    K = _K()
    case, ns, b, m, _, _, _ = shape
    assert K.eval_lin4_supported(b, 4, 64, 128, m, ns)
    wts, img = _lin4_setup()
    x4 = C.input_lin4(b, m, ns, seed=ns, device=DEV)
    out = _lin4(x4)
    assert out.shape == (b, 128, m)
    truth, pre = C.truth_lin4(x4, wts)
    _check_values("lin4<%d> %s" % (ns, case), out, truth, pre, C.plain_fp32("lin4", x4, wts))
    buf = _poisoned(b, 128, m)
    assert _abi_lin4(x4.data_ptr(), img.data_ptr(), buf, b, m, ns) == 0
    assert torch.equal(buf, out)
    _check_invariances(_lin4, x4, out)


def test_tiles_per_wave_query():
    K = _K()
    for c_out in (128, 256):
        for _, ns, b, m, tpw, *_ in C.STORED_SHAPES:
            if ns == 64:
                assert K.eval_stored_tiles_per_wave(b, c_out, m, ns) == 2
        assert K.eval_stored_tiles_per_wave(1, c_out, 1, 64) == 2
        assert K.eval_stored_tiles_per_wave(1, c_out, 2, 16) == 1
    # unsupported shapes: 0
    assert K.eval_stored_tiles_per_wave(1, 192, 256, 16) == 0
    assert K.eval_stored_tiles_per_wave(1, 128, 256, 8) == 0
    assert K.eval_stored_tiles_per_wave(1, 128, 3, 16) == 0
    assert K.eval_stored_tiles_per_wave(0, 128, 256, 16) == 0


def _shifted(img):
    """the same bytes one byte off 16-byte alignment"""
    buf = torch.empty(img.numel() + 16, dtype=torch.uint8, device=DEV)
    off = buf[1:1 + img.numel()]
    off.copy_(img)
    assert off.data_ptr() % 16 == 1
    return off


@pytest.mark.parametrize("why,c_out,m,ns", [("image", 128, 256, 16), ("c_out", 192, 256, 16),
                                            ("ns", 128, 8, 8), ("columns", 128, 3, 16)])
def test_stored_rejections_launch_nothing(why, c_out, m, ns):
    K = _K()
    wts, img = _stored_setup(256 if c_out == 192 else c_out)
    c0, c1, c2 = wts["coeff"]
    if why == "image":
        img = _shifted(img)
    if why == "c_out":
        c2 = (c2[0][:192].contiguous(), c2[1][:192].contiguous())
        assert not K.eval_stored_supported(1, 128, 128, 192, m, ns)
    else:
        assert K.eval_stored_supported(1, 128, 128, c_out, m, ns) == (why == "image")
    y0 = C.input_stored(1, m, ns, device=DEV)
    with pytest.raises(RuntimeError):
        K.eval_stored_pool(y0, c0, img, c1, c2)
    buf = _poisoned(1, 256, max(m, 256))
    assert _abi_stored(y0.data_ptr(), img.data_ptr(), buf, 1, c_out, m, ns) != 0
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


@pytest.mark.parametrize("why,m,ns", [("image", 16, 16), ("ns", 32, 8), ("columns", 6, 16), ("columns", 4, 32)])
def test_lin4_rejections_launch_nothing(why, m, ns):
    K = _K()
    wts, img = _lin4_setup()
    if why == "image":
        img = _shifted(img)
    else:
        assert not K.eval_lin4_supported(1, 4, 64, 128, m, ns)
    x4 = C.input_lin4(1, m, ns, device=DEV)
    with pytest.raises(RuntimeError):
        K.eval_lin4_pool(x4, img, wts["coeff"][1], wts["coeff"][2])
    buf = _poisoned(1, 128, 256)
    assert _abi_lin4(x4.data_ptr(), img.data_ptr(), buf, 1, m, ns) != 0
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
