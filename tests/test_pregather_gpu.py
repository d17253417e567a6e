"""The first shared-MLP layer applied before the gather -- csrc/mlp_pregather.hip: pregather_pack_kernel,
pregather_unpack_kernel, pregather_forward_kernel, pregather_backward_kernel<4 | 8 | 16 | 32> -- kernel by
kernel and run by run.  tests/pregather_cases.py has the shapes, the index patterns, the inputs, the truth, the
measures and their floors; tests/test_pregather_cases.py proves on the CPU that the index rows hold every
class of run the backward stitches and that the rule fails a swapped coefficient, a lost sign and one
dropped entry.

Exact wherever the operation is: pack (one fp32 multiplication per element), unpack (a copy), the forward's
values (one fp32 subtraction per element), the backward on integer data (every sum an integer below 2^24, so
the order of summation plays no part and only the stitching of the runs is left to go wrong), two launches
against one another.  Elsewhere  e(kernel) <= 3 e(plain fp32) + floor  against float64, the floors derived in
the case module; every figure is printed before it is asserted."""
import ctypes
import functools
import importlib

import pytest
import torch

from conftest import load_pkg
import pregather_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = 1                   # hipErrorInvalidValue
IDS = [C.row_id(r) for r in C.INDEX_ROWS]
OVER = (1, 2)                 # the backward's yardstick: plain fp32's worst figure of the cloud


def _K():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


def _E():
    load_pkg()
    return importlib.import_module("pointnet2._ext")


def _dev(t):
    return t.to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _forward_case(row):
    """inputs, the fp32 values and the float64 pairs of one index row: computed once, shared, never written to"""
    inp = C.make_forward_inputs(row)
    y = C.forward_truth(inp["z"], inp["idx"], row[3])
    return inp, y, C.pair_truth64(y)


@functools.lru_cache(maxsize=None)
def _general_case(row):
    inp = C.make_general_backward(row)
    truth, mass, floor_abs = C.general_backward_truth64(inp)
    e32 = C.backward_errors(C.general_backward_plain_fp32(inp), truth, mass)
    return inp, truth, mass, C.backward_floor(mass, floor_abs), e32


def _fly(inp):
    return tuple(_dev(inp[k]) for k in ("y", "dz", "scale", "shift", "mean", "invstd", "coef"))


def _inverse(idx, n):
    inv = _E().group_inverse(idx, n)
    assert inv is not None
    return inv


# ------------------------------------------------------------------ pack and unpack
@pytest.mark.parametrize("s", C.PACK_SCALES, ids=["s1", "s1.25"])
@pytest.mark.parametrize("b,c,n,m", C.pack_shapes())
def test_pack_is_the_concatenation(b, c, n, m, s):
    """pregather_pack == cat([xyz s | new_xyz s ; features | 0]) in fp32 torch, bit for bit (s = 1 and 1 / 0.8,
    SA2's normalisation; every element of the output is compared)"""
    K = _K()
    xyz, new_xyz, feat = C.make_pack_inputs(b, c, n, m)
    got = K.pregather_pack(_dev(xyz), _dev(new_xyz), _dev(feat), s)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (b, 3 + c, n + m)
    assert torch.equal(got.cpu(), C.pack_truth(xyz, new_xyz, feat, s))


@pytest.mark.parametrize("b,c,n,m", C.pack_shapes())
def test_unpack_is_the_slice(b, c, n, m):
    """pregather_unpack_grad == d src_ext[:, 3:, :n], bit for bit"""
    K = _K()
    g = torch.Generator().manual_seed(b + 3 * c + 5 * n + 7 * m)
    dsrc = torch.randn(b, 3 + c, n + m, generator=g)
    got = K.pregather_unpack_grad(_dev(dsrc), n, m)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (b, c, n)
    assert torch.equal(got.cpu(), C.unpack_truth(dsrc, n))


# ------------------------------------------------------------------ forward
def _raw_forward(K, z, idx, n, with_pairs=True):
    """mlp_pregather_forward through the library handle: y and the raw (mean, M2) pairs"""
    b, c, w = z.shape
    m, ns = idx.shape[1], idx.shape[2]
    y = torch.full((b, c, m, ns), float("nan"), device=z.device)
    pairs = torch.full((b, c, 2), float("nan"), device=z.device) if with_pairs else None
    with torch.cuda.device(z.device):
        rc = K._lib.mlp_pregather_forward(b, c, n, m, ns, z.data_ptr(), idx.data_ptr(), y.data_ptr(),
                                          pairs.data_ptr() if with_pairs else None, K._stream(z))
    torch.cuda.synchronize()
    assert rc == 0
    return y, pairs


@pytest.mark.parametrize("row", C.INDEX_ROWS, ids=IDS)
def test_forward_values_and_pairs(row):
    """y == z[:, :, idx] - z[:, :, n + j] in fp32, bit for bit, with and without pairs; the raw (mean, M2) of
    every (cloud, channel) row against float64 on that y under the rule (yardstick: fp32 mean and the sum of
    squares about it; floors: pregather_cases.pair_floors); a constant row has its mean exact and M2 == 0.

    Measured on the MI355X, worst row of each case over its index rows, kernel | plain fp32 (error of the mean
    in units of the row's sigma; of M2 relative), the tiny-noise channel apart:
      case           mean                  M2
      one_quad       0       | 0           0       | 0          (every row constant: exact)
      nine_wgs       6.3e-06 | 9.4e-06     1.8e-06 | 1.6e-07
      pad_mid_lane   2.7e-06 | 1.2e-05     7.2e-06 | 1.7e-07
      no_pad         5.7e-06 | 1.3e-05     8.4e-06 | 2.1e-07
      sa3            2.7e-06 | 1.6e-05     3.7e-06 | 2.0e-07
      limits         2.4e-06 | 1.5e-05     4.7e-06 | 1.4e-07
      wide_groups    5.6e-06 | 2.9e-05     2.9e-07 | 1.3e-07
      tiny-noise row, all cases   mean up to 9.9e-02 | 2.0e+00 (half an ulp of 100 is a tenth of that sigma),
                                  M2 up to 1.2e-07 | 4.2e+00
    M2 costs the shifted form up to 8e-06 where the row's first element is six sigma off its mean -- the floor
    (worst case: 34.5 ULP of M2 + 51.5 ULP of n (shift - mean)^2) allows 2e-04 there; no row needs more than
    0.22 of its bound."""
    K = _K()
    case, b, c, n, m, ns, pats = row
    inp, want, tru = _forward_case(row)
    z, idx = _dev(inp["z"]), _dev(inp["idx"])
    y, pairs = _raw_forward(K, z, idx, n)
    assert torch.equal(y.cpu(), want)
    y2, _ = _raw_forward(K, z, idx, n, with_pairs=False)
    assert torch.equal(y2, y)
    assert torch.equal(K.pregather_forward(z, idx, n), y)
    pairs = pairs.cpu()
    bad = []
    for name, ok, need, e, e32 in C.pair_rule((pairs[:, :, 0], pairs[:, :, 1]), want, tru):
        print("pairs %s %-20s kernel %.2e | plain fp32 %.2e | %.2f of the bound" % (C.row_id(row), name, e, e32, need))
        if not ok:
            bad.append((name, e, e32, need))
    assert not bad, bad
    const = tru[1] == 0
    assert int(const.sum()) >= b
    assert torch.equal(pairs[:, :, 0].double()[const], tru[0][const]) and not bool(pairs[:, :, 1][const].any())


@pytest.mark.parametrize("row", C.INDEX_ROWS, ids=IDS)
def test_forward_batchnorm_coefficients(row):
    """pregather_forward(..., stats=...): mean, invstd, scale, shift and the running statistics of the layer's
    BatchNorm over all clouds, at the bounds test_batchnorm_per_channel_forms (tests/test_gpu_mlp.py) holds the
    other statistics paths to: mean and running mean 1e-6 of max |y|, invstd 1e-5 relative, running variance
    1e-5 of the largest variance; scale and shift follow from the launch's own mean and invstd (1e-5 of their
    largest, + 1e-7: that test's bound between two forms)."""
    K = _K()
    case, b, c, n, m, ns, pats = row
    inp, want, _ = _forward_case(row)
    rm, rv = _dev(inp["rm"]).clone(), _dev(inp["rv"]).clone()
    gamma, beta = _dev(inp["gamma"]), _dev(inp["beta"])
    y, mean, invstd, scale, shift = K.pregather_forward(_dev(inp["z"]), _dev(inp["idx"]), n,
                                                        (gamma, beta, rm, rv, inp["momentum"], inp["eps"]))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), want)
    st = C.batch_stats64(want, inp)
    absmax, mom = float(st["absmax"]), inp["momentum"]
    mean, invstd, scale, shift, rm, rv = (t.double().cpu() for t in (mean, invstd, scale, shift, rm, rv))
    figs = {"mean": float((mean - st["mean"]).abs().max()) / absmax,
            "invstd": float((invstd * (st["var"] + inp["eps"]).sqrt() - 1).abs().max()),
            "running_mean": float((rm - st["running_mean"]).abs().max()) / absmax,
            "running_var": float((rv - st["running_var"]).abs().max()) / max(float(st["var"].max()), 1e-300)}
    print("stats %s: %s" % (C.row_id(row), ", ".join("%s %.2e" % kv for kv in figs.items())))
    assert figs["mean"] <= 1e-6 and figs["invstd"] <= 1e-5 and figs["running_mean"] <= 1e-6
    if float(st["var"].max()) > 0:
        assert figs["running_var"] <= 1e-5
    else:   # every row constant (one point, one group): the unbiased variance is 0 too
        assert float((rv - (1 - mom) * inp["rv"].double()).abs().max()) <= 1e-6
    sc_own = inp["gamma"].double() * invstd
    sh_own = inp["beta"].double() - mean * scale
    assert float((scale - sc_own).abs().max()) <= 1e-5 * float(sc_own.abs().max()) + 1e-7
    assert float((shift - sh_own).abs().max()) <= 1e-5 * float(sh_own.abs().max()) + 1e-7
    assert all(bool(torch.isfinite(t).all()) for t in (mean, invstd, scale, shift, rm, rv))


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("row", C.INDEX_ROWS, ids=IDS)
def test_backward_exact_form(row):
    """scale 1, shift 0, coef (1, 0, 0), integer dz: dz_ext[:, :, :n] == the int64 scatter-add of the gated dz
    over idx and dz_ext[:, :, n + j] == minus the group sum, as numbers, on every case and every pattern"""
    K = _K()
    case, b, c, n, m, ns, pats = row
    inp = C.make_exact_backward(row)
    want = C.exact_backward_truth(inp)
    idx = _dev(inp["idx"])
    got = K.pregather_backward(_fly(inp), _inverse(idx, n), n)
    torch.cuda.synchronize()
    got = got.cpu()
    assert tuple(got.shape) == (b, c, n + m)
    wrong = (got.double() != want.double())
    if bool(wrong.any()):
        cl, ch, col = (int(v) for v in wrong.nonzero()[0])
        where = "point %d" % col if col < n else "group %d" % (col - n)
        raise AssertionError("%d of %d sums differ; first: cloud %d (%s) channel %d %s: %r, not %d"
                             % (int(wrong.sum()), wrong.numel(), cl, pats[cl], ch, where, float(got[cl, ch, col]),
                                int(want[cl, ch, col])))
    assert torch.equal(got, want.float())


@pytest.mark.parametrize("row", C.INDEX_ROWS, ids=IDS)
def test_backward_general_form(row):
    """random scale, shift, mean, invstd, coef (|mean| invstd = 40 on every fourth channel) against the float64
    scatter of the unfolded a (g - c1 - (y - mu) is c2); measure |got - truth| / mass per output, mass = the
    run's sum of |a g| + |q y| + |p|; rule per output with the cloud's worst plain-fp32 figure as yardstick and
    the fold's floor (at most 3 ULP of the mass).  An unreferenced point is exactly 0.  Two launches on one
    inverse and a launch on a second, independently built inverse give the same bits.

    Measured on the MI355X, worst output of each case over its index rows, kernel | plain fp32 (CPU
    scatter_add_ in index order), in units of the output's mass; the floor is 3.6e-07 at most:
      one_quad 1.2e-07 | 6.4e-08   nine_wgs 1.0e-07 | 1.6e-07   pad_mid_lane 1.9e-07 | 2.6e-07
      no_pad   1.5e-07 | 1.9e-07   sa3      2.3e-07 | 6.9e-07   limits       2.3e-07 | 5.7e-07
      wide_groups 2.9e-07 | 5.9e-07;  no output needs more than 0.38 of its bound."""
    K = _K()
    case, b, c, n, m, ns, pats = row
    inp, truth, mass, floor, e32 = _general_case(row)
    idx, fly = _dev(inp["idx"]), _fly(inp)
    inv = _inverse(idx, n)
    got = K.pregather_backward(fly, inv, n)
    again = K.pregather_backward(fly, inv, n)
    inv2 = _inverse(idx.clone(), n)
    third = K.pregather_backward(fly, inv2, n)
    torch.cuda.synchronize()
    e = C.backward_errors(got.cpu(), truth, mass)
    ok, need, worst, worst32 = C.within(e, e32, floor, OVER)
    print("backward %s kernel %.2e | plain fp32 %.2e | floor %.2e | %.2f of the bound"
          % (C.row_id(row), worst, worst32, float(floor.max()), need))
    assert ok, (worst, worst32, need)
    dead = mass == 0
    assert not bool(got.cpu()[dead].any())
    assert torch.equal(again, got) and torch.equal(third, got)


# ------------------------------------------------------------------ the gate
def test_gate_is_the_formula():
    K = _K()
    for case, b, c, n, m, ns in C.SHAPES:
        assert K.pregather_supported(b, c, n, m, ns) and C.gate(b, c, n, m, ns), case
    for what, b, c, n, m, ns in C.OUTSIDE:
        assert not K.pregather_supported(b, c, n, m, ns) and not C.gate(b, c, n, m, ns), what
    for shape in ((0, 4, 1, 1, 4), (1, 0, 1, 1, 4), (1, 4, 0, 1, 4), (1, 4, 1, 0, 4), (1, 4, 4096, 4096, 8),
                  (1, 65536, 1, 1, 4), (1, 4, 1, 1, 1), (8, 128, 2048, 1024, 32), (8, 256, 1024, 512, 16)):
        assert K.pregather_supported(*shape) == C.gate(*shape), shape


@pytest.mark.parametrize("what,b,c,n,m,ns", C.OUTSIDE, ids=[o[0].replace(" ", "") for o in C.OUTSIDE])
def test_outside_the_gate_nothing_is_launched(what, b, c, n, m, ns):
    """the forward and backward wrappers raise; the entry points return hipErrorInvalidValue before any launch:
    the output buffers keep their fill"""
    K = _K()
    z = torch.zeros(b, c, n + m, device=DEV)
    idx = torch.zeros(b, m, ns, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        K.pregather_forward(z, idx, n)
    y = torch.full((b, c, m, ns), 7.0, device=DEV)
    with torch.cuda.device(z.device):
        rc = K._lib.mlp_pregather_forward(b, c, n, m, ns, z.data_ptr(), idx.data_ptr(), y.data_ptr(), None,
                                          K._stream(z))
    assert rc == INVALID
    one, zero = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    coef = torch.stack([one, zero, zero], dim=1).contiguous()
    fly = (y, torch.ones_like(y), one, zero, zero.clone(), one.clone(), coef)
    entries = int(K._lib.pn2_group_inverse_entries(m, ns))
    inverse = torch.full((b, entries), -1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        K.pregather_backward(fly, inverse, n)
    out = torch.full((b, c, n + m), 7.0, device=DEV)
    op = K._grad_operand(fly=fly)
    with torch.cuda.device(z.device):
        rc = K._lib.mlp_pregather_backward(b, c, n, m, ns, ctypes.byref(op), inverse.data_ptr(), out.data_ptr(),
                                           K._stream(z))
    torch.cuda.synchronize()
    assert rc == INVALID
    assert bool((y == 7.0).all()) and bool((out == 7.0).all())
