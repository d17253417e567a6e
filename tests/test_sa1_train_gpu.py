"""Set abstraction 1's training forward -- csrc/mlp_chain.hip (chain_prep_kernel, chain_lin4_kernel<4, NS, FULL>
for NS = 16 / 32 / 64 as statistics pass and full pass, chain_finalize_kernel) and csrc/mlp_first4.hip
(moments, BatchNorm from the moments, the first layer's weight gradient) -- against float64 torch, edge by
edge.  tests/sa1_train_cases.py has the shapes, the inputs, the truth, the measures and their floors;
tests/test_sa1_train_cases.py proves on the CPU that the inputs meet their conditions and that the bound fails
a kernel that loses one of its six partial products.

Bound, everywhere a kernel is compared with float64: e(kernel) <= 3 e(plain fp32 torch on the same inputs) +
what the fp32 format alone resolves (sa1_train_cases: tensor_floors, stat_floors, own_floors, grad_floors).
No fixed tolerance appears below; mlp_chain_finalize and first4_moments, whose sums are in double, are held to
the rounding of their fp32 outputs plus n 2^-53 on the double sums.  Every figure is printed before it is
asserted ("SA1's training forward against float64", has the measured table).
Bit-exact properties are asserted with torch.equal; the entry points are also called through the library
handle with the test's own buffers inside a NaN-filled arena."""
import ctypes
import functools
import importlib
import math

import pytest
import torch

from conftest import load_pkg
import sa1_train_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024                  # 32-bit words between the buffers of the arena
FILL = 0x7fc0dead             # a NaN no computation produces
INVALID = 1                   # hipErrorInvalidValue
IDS = ["%s-ns%d" % (s[0], s[1]) for s in C.CHAIN_SHAPES]


def _K():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


@functools.lru_cache(maxsize=None)
def _case(row):
    """inputs on the device, truth, yardstick and the checked conditions of one row: computed once, shared,
    never written to"""
    case, ns, b, m, tpc, wgs, seed, momentum, running = row
    inp = C.make_chain_inputs(b, m, ns, seed, momentum, running, device=DEV)
    tru = C.truth64(inp)
    return inp, tru, C.plain_fp32(inp), C.check_inputs(inp, tru)


def _wrapper(K, inp, store=True, store_last=True):
    """chain_lin4_forward on fresh copies of the running statistics -> dict as sa1_train_cases._layers"""
    run = [inp[k].clone() for k in ("rm1", "rv1", "rm2", "rv2")] if inp["running"] else [None] * 4
    y2, c2, y3, c3, ext = K.chain_lin4_forward(
        inp["x4"], inp["w0"], (inp["sc0"], inp["sh0"]),
        (inp["w1"], inp["g1"], inp["be1"], run[0], run[1], inp["momentum"], inp["eps"]),
        (inp["w2"], inp["g2"], inp["be2"], run[2], run[3], inp["momentum"], inp["eps"]),
        store=store, store_last=store_last)
    torch.cuda.synchronize()
    return {"y2": y2, "y3": y3, "stats2": tuple(c2), "stats3": tuple(c3), "ext": ext,
            "running2": (run[0], run[1]) if inp["running"] else None,
            "running3": (run[2], run[3]) if inp["running"] else None}


def _report(tag, rows, bad):
    for name, ok, need, e, e32 in rows:
        print("%s %-22s kernel %.2e | plain fp32 %.2e | %.2f of the bound" % (tag, name, e, e32, need))
        if not ok:
            bad.append((name, e, e32, need))


def _ext_is_the_first_winner(y3, ext, gamma2):
    """ext[0] is the stored output gathered at ext[1]; ext[1] is the FIRST index attaining the maximum of
    sign(gamma2) y within the group -- exactly"""
    idx = ext[1].view(torch.int32)
    ns = y3.shape[3]
    assert int(idx.min()) >= 0 and int(idx.max()) < ns
    assert torch.equal(ext[0], torch.gather(y3, 3, idx.long().unsqueeze(-1)).squeeze(-1))
    _, first = C.first_winner(y3, gamma2)
    assert torch.equal(idx.long(), first)


@pytest.mark.parametrize("row", C.CHAIN_SHAPES, ids=IDS)
def test_chain_vs_float64(row):
    K = _K()
    inp, tru, p32, info = _case(row)
    case, ns, b, m = row[:4]
    tag = "chain %s ns %d (%d, %d)" % (case, ns, b, m)
    assert int(K._lib.mlp_chain_lin4_parts(b, m * ns, 128, ns, None)) == row[5]
    got = _wrapper(K, inp)
    bad = []
    # ---- both stored outputs, both layers' coefficients, the running statistics: against the truth
    _report(tag, C.compare_chain(got, p32, tru, inp), bad)
    # ---- the same coefficients against the float64 statistics of the kernel's OWN stored outputs; yardstick:
    # fp32 torch mean / var of that same tensor.  (Layer 2's pairs come from the T-form statistics pass, its
    # stored values from the N form of the full pass.)
    for layer, (g, be) in ((2, ("g1", "be1")), (3, ("g2", "be2"))):
        y = got["y%d" % layer]
        st64 = C.stats_of(y, inp[g], inp[be], inp["eps"], torch.float64)
        st32 = C.stats_of(y, inp[g], inp[be], inp["eps"], torch.float32)
        e = C.stat_errors(got["stats%d" % layer], st64)
        e32 = C.stat_errors(tuple(st32[k] for k in ("mean", "invstd", "scale", "shift")), st64)
        fl = C.own_floors(st64)
        _report(tag, [("own %s%d" % (k, layer),) + C.within(e[k], e32[k], fl[k])
                      for k in ("mean", "invstd", "scale", "shift")], bad)
    # ---- the constant channels: mean 0, invstd = 1 / sqrt(eps) rounded, everything finite
    inv0 = torch.tensor(1.0 / math.sqrt(inp["eps"]), dtype=torch.float32)
    for layer, ch in ((2, C.ZERO_ROW1), (3, C.ZERO_ROW2)):
        mean, invstd, scale, shift = got["stats%d" % layer]
        assert float(mean[ch]) == 0.0 and float(invstd[ch]) == float(inv0)
        assert not bool(got["y%d" % layer][:, ch].any())
        assert all(bool(torch.isfinite(t).all()) for t in (mean, invstd, scale, shift, got["y%d" % layer]))
    # ---- the extrema planes against the kernel's own stored layer-3 output, exactly: every planted tie, the
    # border of two ns = 16 groups inside a tile
    y3, ext = got["y3"], got["ext"]
    _ext_is_the_first_winner(y3, ext, inp["g2"])
    idx = ext[1].view(torch.int32).long()
    for _, later in C.TIES + ((C.TIE_64,) if ns == 64 else ()):
        assert not bool((idx[:, :, ::C.TIE_EVERY] == later).any()), "a later copy won"
    assert bool((idx[:, C.ZERO_ROW2] == 0).all())
    # ---- the pooled tensor
    c3 = got["stats3"]
    pooled, argmax, ymax = K.pool_from_extrema(ext, c3[2], c3[3])
    torch.cuda.synchronize()
    assert torch.equal(argmax.long(), idx) and torch.equal(ymax, ext[0])
    var_p = tru["pooled"].var(dim=(0, 2), unbiased=False)
    eg, ec = C.tensor_errors(pooled, tru["pooled"], var_p)
    pg, pc = C.tensor_errors(p32["pooled"], tru["pooled"], var_p)
    fg, fc = C.tensor_floors(tru["pooled"], var_p)
    _report(tag, [("pooled global",) + C.within(eg, pg, fg), ("pooled channel",) + C.within(ec, pc, fc)], bad)
    for ch in (C.GAMMA2_ZERO_CH, C.ZERO_ROW2):
        assert bool((pooled[:, ch] == torch.relu(inp["be2"][ch])).all())
    assert bool(torch.isfinite(pooled).all())
    # the arg-max differs from float64's only where the rivals are within the bound of y3 (both may err)
    v64 = tru["y3"] * C.pool_sign(inp["g2"]).double().view(1, -1, 1, 1)
    _, first64 = C.first_winner(tru["y3"], inp["g2"])
    var3 = tru["stats3"]["var"]
    _, e32c = C.tensor_errors(p32["y3"], tru["y3"], var3)
    _, floor_c = C.tensor_floors(tru["y3"], var3)
    bound_abs = ((C.RATIO * float(e32c.max()) + floor_c) * var3.sqrt()).view(1, -1, 1)
    gap = torch.gather(v64, 3, first64.unsqueeze(-1)).squeeze(-1) - torch.gather(v64, 3, idx.unsqueeze(-1)).squeeze(-1)
    differs = idx != first64
    print("%s arg-max differs from float64's in %d of %d groups (%d near-tied in float64), worst gap / bound %.2f"
          % (tag, int(differs.sum()), differs.numel(), int(info["near"].sum()),
             float((gap / (2 * bound_abs).clamp_min(1e-300))[differs].max()) if bool(differs.any()) else 0.0))
    assert bool((gap >= 0).all()) and bool((gap[differs] <= (2 * bound_abs).expand_as(gap)[differs]).all())
    assert not bad, bad


@pytest.mark.parametrize("row", C.CHAIN_SHAPES, ids=IDS)
def test_chain_storing_or_not_and_twice(row):
    """store=False and store_last=False leave the same coefficients, running statistics and extrema as the
    storing run, and so does a second storing run -- the same bits"""
    K = _K()
    inp = _case(row)[0]
    base = _wrapper(K, inp)
    for kw in ({}, {"store_last": False}, {"store": False}):
        other = _wrapper(K, inp, **kw)
        assert (other["y2"] is None) == (kw.get("store") is False)
        assert (other["y3"] is None) == bool(kw)
        for layer in (2, 3):
            for mine, theirs in zip(base["stats%d" % layer], other["stats%d" % layer]):
                assert torch.equal(mine, theirs), (kw, layer)
            if inp["running"]:
                for mine, theirs in zip(base["running%d" % layer], other["running%d" % layer]):
                    assert torch.equal(mine, theirs), (kw, layer)
        assert torch.equal(base["ext"].view(torch.int32), other["ext"].view(torch.int32)), kw
        for name in ("y2", "y3"):
            if other[name] is not None:
                assert torch.equal(base[name], other[name]), (kw, name)


class Arena(object):
    """One int32 tensor filled with FILL; take(n) hands out n 32-bit words, 16-byte aligned, GUARD words
    after whatever came before"""

    def __init__(self, words):
        self.raw = torch.full((words,), FILL, dtype=torch.int32, device=DEV)
        assert self.raw.data_ptr() % 16 == 0
        self.at, self.taken = GUARD, []

    def take(self, n, name, dtype=torch.float32):
        assert n % 4 == 0 and self.at + n + GUARD <= self.raw.numel(), name
        view = self.raw[self.at:self.at + n]
        self.taken.append((name, self.at, n))
        self.at += n + GUARD
        return view.view(dtype)

    def guards_intact(self):
        mask = torch.ones_like(self.raw, dtype=torch.bool)
        for _, lo, n in self.taken:
            mask[lo:lo + n] = False
        return bool((self.raw[mask] == FILL).all())

    def unwritten(self):
        """names of the buffers in which a word still holds FILL"""
        return [name for name, lo, n in self.taken if bool((self.raw[lo:lo + n] == FILL).any())]

    def untouched(self):
        return bool((self.raw == FILL).all())


def _chain_buffers(K, b, m, ns, parts=None):
    r = m * ns
    parts = parts if parts is not None else int(K._lib.mlp_chain_lin4_parts(b, r, 128, ns, None))
    img_words = int(K._lib.mlp_chain_lin4_image_bytes()) // 4
    sizes = (("img", img_words), ("pairs2", parts * 64 * 2), ("pairs3", parts * 128 * 2), ("y2", b * 64 * r),
             ("y3", b * 128 * r), ("ext", 2 * b * 128 * m))
    arena = Arena(sum(n for _, n in sizes) + GUARD * (len(sizes) + 1))
    return arena, {name: arena.take(n, name) for name, n in sizes}, parts


def _p(t):
    return t.data_ptr() if t is not None else None


def _prepare(K, inp, img):
    with torch.cuda.device(DEV):
        return int(K._lib.mlp_chain_lin4_prepare(inp["w0"].data_ptr(), inp["sc0"].data_ptr(), inp["sh0"].data_ptr(),
                                                 inp["w1"].data_ptr(), inp["w2"].data_ptr(), _p(img), K._stream(inp["x4"])))


def _stats(K, b, r, ns, x4, img, pairs2):
    with torch.cuda.device(DEV):
        rc = int(K._lib.mlp_chain_lin4_stats(b, r, ns, _p(x4), img, _p(pairs2), K._stream(pairs2 if x4 is None else x4)))
        torch.cuda.synchronize()
    return rc


def _forward(K, b, r, ns, x4, img, sc2, sh2, g2, y2, y3, pairs3, ext):
    """y3 and img as addresses (the refusals shift them), the others as tensors or None"""
    with torch.cuda.device(DEV):
        rc = int(K._lib.mlp_chain_lin4_forward(b, r, ns, _p(x4), img, _p(sc2), _p(sh2), _p(g2), _p(y2), y3, _p(pairs3),
                                               _p(ext), K._stream(sc2)))
        torch.cuda.synchronize()
    return rc


def _finalize(K, c, parts, n_part, pairs, gamma, beta, eps, momentum, rm, rv):
    out = torch.full((4, c), float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        rc = int(K._lib.mlp_chain_finalize(c, parts, n_part, pairs.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                           float(eps), float(momentum), _p(rm), _p(rv), out[0].data_ptr(),
                                           out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), K._stream(pairs)))
        torch.cuda.synchronize()
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("row", [s for s in C.CHAIN_SHAPES if s[0] == "three_wg"], ids=["ns16", "ns32", "ns64"])
def test_chain_entry_points_inside_an_arena(row):
    """prepare, statistics pass, finalize, full pass, finalize through the library handle: img, both pairs
    buffers, both raw outputs and ext are exactly their documented sizes inside one NaN-filled arena; no guard
    word changes, no output word stays NaN, and the results are the wrapper's bits"""
    K = _K()
    inp = _case(row)[0]
    case, ns, b, m = row[:4]
    r = m * ns
    arena, buf, parts = _chain_buffers(K, b, m, ns)
    assert parts == row[5] and all(t.data_ptr() % 16 == 0 for t in buf.values())
    assert _prepare(K, inp, buf["img"]) == 0
    assert _stats(K, b, r, ns, inp["x4"], buf["img"].data_ptr(), buf["pairs2"]) == 0
    c2 = _finalize(K, 64, parts, C.COLS_PER_PART, buf["pairs2"], inp["g1"], inp["be1"], inp["eps"], inp["momentum"], None, None)
    assert _forward(K, b, r, ns, inp["x4"], buf["img"].data_ptr(), c2[2], c2[3], inp["g2"], buf["y2"], buf["y3"].data_ptr(),
                    buf["pairs3"], buf["ext"]) == 0
    c3 = _finalize(K, 128, parts, C.COLS_PER_PART, buf["pairs3"], inp["g2"], inp["be2"], inp["eps"], inp["momentum"], None, None)
    assert arena.guards_intact(), "written outside a buffer"
    assert arena.unwritten() == [], "words never written"
    assert not bool(torch.isnan(c2).any()) and not bool(torch.isnan(c3).any())
    got = _wrapper(K, inp)
    assert torch.equal(got["y2"].view(-1), buf["y2"]) and torch.equal(got["y3"].view(-1), buf["y3"])
    assert torch.equal(got["ext"].view(-1).view(torch.int32), buf["ext"].view(torch.int32))
    for mine, theirs in zip(tuple(c2) + tuple(c3), got["stats2"] + got["stats3"]):
        assert torch.equal(mine, theirs)


@pytest.mark.parametrize("row", C.CHAIN_SHAPES, ids=IDS)
def test_chain_moves_with_its_columns(row):
    """With layer 2's coefficients held fixed (the full pass through the library handle): permuting the
    samples inside the groups permutes the stored columns and maps the extrema's indices; rolling the groups
    of a cloud by 1 and by 5 moves the stored columns, the winning values and their indices with them; a cloud
    launched alone gives the stored columns and extrema it gives among its neighbours.  torch.equal."""
    K = _K()
    inp = _case(row)[0]
    case, ns, b, m = row[:4]
    r = m * ns
    img = torch.empty(int(K._lib.mlp_chain_lin4_image_bytes()), dtype=torch.uint8, device=DEV)
    assert _prepare(K, inp, img) == 0
    coeff = _wrapper(K, inp, store=False)["stats2"]
    sc2, sh2 = coeff[2].clone(), coeff[3].clone()

    def run(x4):
        bb = x4.shape[0]
        parts = int(K._lib.mlp_chain_lin4_parts(bb, r, 128, ns, None))
        y2 = torch.full((bb, 64, m, ns), float("nan"), device=DEV)
        y3 = torch.full((bb, 128, m, ns), float("nan"), device=DEV)
        pairs3 = torch.empty((parts, 128, 2), device=DEV)
        ext = torch.full((2, bb, 128, m), float("nan"), device=DEV)
        assert _forward(K, bb, r, ns, x4, img.data_ptr(), sc2, sh2, inp["g2"], y2, y3.data_ptr(), pairs3, ext) == 0
        _ext_is_the_first_winner(y3, ext, inp["g2"])
        return y2, y3, ext

    y2, y3, ext = run(inp["x4"])
    # samples permuted inside every group
    perm = torch.randperm(ns, generator=torch.Generator().manual_seed(ns + m)).to(DEV)
    p2, p3, pext = run(inp["x4"][:, :, :, perm].contiguous())
    assert torch.equal(p2, y2[:, :, :, perm]) and torch.equal(p3, y3[:, :, :, perm])
    assert torch.equal(pext[0], ext[0])
    # (the winner's old position holds the winning value; among tied columns the first in the NEW order wins,
    # which _ext_is_the_first_winner has checked inside run)
    old = perm[pext[1].view(torch.int32).long()]
    assert torch.equal(torch.gather(y3, 3, old.unsqueeze(-1)).squeeze(-1), ext[0])
    # groups rolled inside their clouds
    for shift in (1, 5):
        r2, r3, rext = run(torch.roll(inp["x4"], shifts=shift, dims=2).contiguous())
        assert torch.equal(r2, torch.roll(y2, shifts=shift, dims=2)) and torch.equal(r3, torch.roll(y3, shifts=shift, dims=2))
        assert torch.equal(rext.view(torch.int32), torch.roll(ext, shifts=shift, dims=3).view(torch.int32))
    # one cloud alone
    if b > 1:
        a2, a3, aext = run(inp["x4"][1:2].contiguous())
        assert torch.equal(a2, y2[1:2]) and torch.equal(a3, y3[1:2])
        assert torch.equal(aext.view(torch.int32), ext[:, 1:2].contiguous().view(torch.int32))


# ------------------------------------------------------------------ mlp_chain_finalize on its own
FIN_PARTS = (1, 2, 255, 256, 257, 768, 769, 1023, 1024, 1029, 2053)


@pytest.mark.parametrize("parts", FIN_PARTS)
@pytest.mark.parametrize("c", [1, 64, 128])
def test_chain_finalize_vs_float64(c, parts):
    """Synthetic equal-count pairs, n_part = 256: means at 1000 +- 1 (the kernel sums around the first part's
    mean), the last channel's pairs all equal with M2 = 0; running statistics given and null.  parts walks the
    plain loop (<= 768), the first lane of the four-wide loop (769), and both loops one after the other.
    Tolerance: the rounding of the fp32 outputs (2^-24 per fp32 operation) + parts 2^-53 on the double sums."""
    K = _K()
    n_part = 256
    g = torch.Generator().manual_seed(1000 * c + parts)
    pairs = torch.stack([1000.0 + 2 * torch.rand(parts, c, generator=g) - 1,
                         n_part * (0.5 + torch.rand(parts, c, generator=g))], dim=2)
    flat = c - 1
    pairs[:, flat, 0] = 1000.5
    pairs[:, flat, 1] = 0.0
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::5] *= -1
    beta, rm0, rv0 = torch.randn(c, generator=g) * 0.3, torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    pairs, gamma, beta, rm0, rv0 = (t.float().contiguous().to(DEV) for t in (pairs, gamma, beta, rm0, rv0))
    eps, mom = C.f32(C.EPS), C.f32(0.37)
    want = C.finalize64(pairs, n_part, gamma, beta, eps, mom, rm0, rv0)
    rm, rv = rm0.clone(), rv0.clone()
    out = _finalize(K, c, parts, n_part, pairs, gamma, beta, eps, mom, rm, rv)
    out_null = _finalize(K, c, parts, n_part, pairs, gamma, beta, eps, mom, None, None)
    assert torch.equal(out, out_null)
    mean, invstd, scale, shift = (t.double() for t in out)
    # the kernel's sums, around the first part's mean
    u, dbl = 2.0 ** -24, parts * 2.0 ** -53
    p = pairs.double()
    d = p[:, :, 0] - p[0:1, :, 0]
    s1, s2, sm2 = d.sum(0), (d * d).sum(0), p[:, :, 1].sum(0)
    n = float(parts) * n_part
    m2 = want["var"] * n
    amplified = sm2 + n_part * (s2 + s1 * s1 / parts)
    tol_mean = u * want["mean"].abs() + dbl * (d.abs().mean(0) + want["mean"].abs())
    rel_inv = u + dbl * amplified / (m2 + n * eps)
    rel_scale = rel_inv + u
    tol_shift = u * (want["shift"].abs() + (want["mean"] * want["scale"]).abs()) + tol_mean * want["scale"].abs() \
        + want["mean"].abs() * rel_scale * want["scale"].abs()
    keep = 1 - mom
    tol_rm = u * (2 * (keep * rm0.double()).abs() + (mom * want["mean"]).abs() + want["running_mean"].abs()) + mom * tol_mean
    unbiased = m2 / (n - 1.0)
    tol_rv = u * (2 * (keep * rv0.double()).abs() + 2 * mom * unbiased + want["running_var"].abs()) \
        + mom * dbl * amplified / (n - 1.0)
    figures = (("mean", (mean - want["mean"]).abs(), tol_mean),
               ("invstd", (invstd / want["invstd"] - 1).abs(), rel_inv),
               ("scale", (scale / want["scale"] - 1).abs(), rel_scale),
               ("shift", (shift - want["shift"]).abs(), tol_shift),
               ("running_mean", (rm.double() - want["running_mean"]).abs(), tol_rm),
               ("running_var", (rv.double() - want["running_var"]).abs(), tol_rv))
    bad = []
    for name, err, tol in figures:
        worst = float((err / tol).max())
        print("finalize c %d parts %d %-12s worst error %.2e, %.2f of its tolerance" % (c, parts, name, float(err.max()), worst))
        if not bool((err <= tol).all()):
            bad.append((name, worst))
    # the channel whose pairs are all equal: its mean is that value, its variance exactly 0
    assert float(out[0][flat]) == 1000.5 and float(out[1][flat]) == float(torch.tensor(1.0 / math.sqrt(eps), dtype=torch.float32))
    assert not bad, bad


# ------------------------------------------------------------------ the first layer
@pytest.mark.parametrize("b,r", C.MOMENT_SHAPES)
def test_first4_moments_and_bn_vs_float64(b, r):
    """The 14 moments against float64 sums of the fp32 input (n 2^-53 sum |term| each: the products of two fp32
    values are exact in double), and first4_bn on them against the float64 BatchNorm of W x -- mean, invstd,
    scale, shift, running statistics -- under the rule; yardstick: the fp32 BatchNorm of the fp32 W x."""
    K = _K()
    x = C.make_moment_input(b, r, device=DEV)
    n = b * r
    mom = K.first4_moments(x)
    torch.cuda.synchronize()
    got = mom.view(-1, 14).sum(0)
    want, mag = C.moments64(x)
    err, tol = (got - want).abs(), n * 2.0 ** -53 * mag
    print("first4_moments (%d, %d): worst error / tolerance %.3f" % (b, r, float((err / tol).max())))
    assert bool((err <= tol).all()), (err / tol).tolist()
    w, gamma, beta, rm0, rv0 = C.make_bn_first4(device=DEV)
    eps, momentum = C.f32(C.EPS), C.f32(0.1)
    rm, rv = rm0.clone(), rv0.clone()
    out = K.first4_bn(mom, n, w, gamma, beta, rm, rv, momentum, eps)
    torch.cuda.synchronize()
    st64, y64, run64 = C.first4_bn_stats(x, w, gamma, beta, rm0, rv0, momentum, eps, torch.float64)
    with C._tf32_off():
        st32, _, run32 = C.first4_bn_stats(x, w, gamma, beta, rm0, rv0, momentum, eps, torch.float32)
    e = C.stat_errors(out, st64)
    e32 = C.stat_errors(tuple(st32[k] for k in ("mean", "invstd", "scale", "shift")), st64)
    fl = C.stat_floors(y64, st64)
    rows = [(k,) + C.within(e[k], e32[k], fl[k]) for k in ("mean", "invstd", "scale", "shift")]
    er, er32 = C.running_errors((rm, rv), run64, st64["var"]), C.running_errors(run32, run64, st64["var"])
    rows.append(("running_mean",) + C.within(er[0], er32[0], C.ULP + momentum * fl["mean"]))
    rows.append(("running_var",) + C.within(er[1], er32[1], C.ULP + 2 * momentum * fl["invstd"]))
    bad = []
    _report("first4_bn (%d, %d)" % (b, r), rows, bad)
    # the all-zero weight row: mean 0, invstd 1 / sqrt(eps) rounded
    assert float(out[0][C.ZERO_ROW1]) == 0.0
    assert float(out[1][C.ZERO_ROW1]) == float(torch.tensor(1.0 / math.sqrt(eps), dtype=torch.float32))
    assert all(bool(torch.isfinite(t).all()) for t in tuple(out) + (rm, rv))
    # without running buffers: the same coefficients
    out2 = K.first4_bn(mom, n, w, gamma, beta, None, None, momentum, eps)
    assert all(torch.equal(a, b_) for a, b_ in zip(out, out2))
    assert not bad, bad


@pytest.mark.parametrize("b,r", C.FIRST4_SHAPES)
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_wgrad_first4_vs_float64(b, r, training):
    """dW of the first layer against the float64 autograd of conv -> BatchNorm -> ReLU; with the moments handed
    in and with None the same bits.  Relative L2 and max over the range under the rule; yardstick: einsum of
    the fp32 dy and x."""
    K = _K()
    inp = C.make_first4_inputs(b, r, training, device=DEV)
    info = C.check_first4_inputs(inp)
    assert int(K._lib.mlp_wgrad_first4_workspace_bytes(b, r)) == \
        (4 * (b * C.first4_slices(b, r)[0] + 1) * 256 + 7) // 8 * 8 + 8 * 256 * 14
    fly = (None, inp["dz"], inp["scale"], inp["shift"], inp["mean"], inp["invstd"], inp["coef"])
    got = K.wgrad_first4(inp["w"], inp["x"], fly)
    again = K.wgrad_first4(inp["w"], inp["x"], fly, moments=K.first4_moments(inp["x"]))
    torch.cuda.synchronize()
    assert got is not None and torch.equal(got, again)
    truth = C.first4_truth64(inp)
    e, e32, fl = C.grad_errors(got, truth), C.grad_errors(C.first4_plain_fp32(inp), truth), C.grad_floors(truth)
    bad = []
    _report("wgrad_first4 (%d, %d) %s excluded %.1e" % (b, r, "train" if training else "eval", info["excluded"]),
            [("rel-L2",) + C.within(e[0], e32[0], fl[0]), ("max/range",) + C.within(e[1], e32[1], fl[1])], bad)
    assert not bad, bad


# ------------------------------------------------------------------ refusals
def _refusal_buffers(K):
    # as large as any reading of the refused shapes could want: a call that ran after all stays inside
    return _chain_buffers(K, 1, 32, 16, parts=8)


@pytest.mark.parametrize("what", ["r % 256 != 0", "ns = 8", "x4 null", "img null", "pairs null", "img off by 4 bytes",
                                  "y3 off by 4 bytes"])
def test_chain_refusals(what):
    """hipErrorInvalidValue from both passes, nothing launched: every buffer still holds its fill pattern"""
    K = _K()
    row = C.CHAIN_SHAPES[0]
    inp = _case(row)[0]
    b, m, ns = {"r % 256 != 0": (1, 8, 16), "ns = 8": (1, 32, 8)}.get(what, (1, 16, 16))
    r = m * ns
    arena, buf, _ = _refusal_buffers(K)
    img = torch.zeros(int(K._lib.mlp_chain_lin4_image_bytes()) + 16, dtype=torch.uint8, device=DEV)
    assert _prepare(K, inp, img) == 0
    if what in ("r % 256 != 0", "ns = 8"):
        assert int(K._lib.mlp_chain_lin4_parts(b, r, 128, ns, None)) == 0
    x4 = None if what == "x4 null" else torch.zeros(b, 4, m, ns, device=DEV)
    img_at = {"img null": None, "img off by 4 bytes": img.data_ptr() + 4}.get(what, img.data_ptr())
    y3_at = buf["y3"].data_ptr() + (4 if what == "y3 off by 4 bytes" else 0)
    pairs2 = None if what == "pairs null" else buf["pairs2"]
    pairs3 = None if what == "pairs null" else buf["pairs3"]
    sc2, sh2 = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    if what != "y3 off by 4 bytes":   # (the statistics pass has no y3)
        assert _stats(K, b, r, ns, x4, img_at, pairs2) == INVALID
    assert _forward(K, b, r, ns, x4, img_at, sc2, sh2, inp["g2"], buf["y2"], y3_at, pairs3, buf["ext"]) == INVALID
    assert arena.untouched(), "written by a refused call"
    if what == "img off by 4 bytes":
        assert _prepare(K, inp, img[4:]) == INVALID


def test_first4_refusals():
    """r % 4 != 0 and null pointers: an error code, dw and the workspace still at their fill pattern"""
    K = _K()
    lib = K._lib
    b, r = 1, 6
    inp = C.make_first4_inputs(1, 8, True, device=DEV)
    arena = Arena(4 * GUARD + 256 + 8192)
    dw, ws = arena.take(256, "dw"), arena.take(8192, "workspace")
    assert 4 * 8192 >= int(lib.mlp_wgrad_first4_workspace_bytes(1, 8))
    names = ("w", "x", "dz", "scale", "shift", "mean", "invstd", "coef")

    def call(r_, **null):
        ptr = {k: inp[k].data_ptr() for k in names}
        ptr.update(dw=dw.data_ptr(), ws=ws.data_ptr())
        ptr.update({k: None for k in null})
        with torch.cuda.device(DEV):
            rc = int(lib.mlp_wgrad_first4(b, r_, ptr["w"], ptr["x"], ptr["dz"], ptr["scale"], ptr["shift"], ptr["mean"],
                                          ptr["invstd"], ptr["coef"], None, ptr["dw"], ptr["ws"], K._stream(inp["x"])))
            torch.cuda.synchronize()
        return rc

    assert call(r) == INVALID and arena.untouched()
    for k in names + ("dw", "ws"):
        assert call(8, **{k: True}) == INVALID, k
        assert arena.untouched(), k
    x6 = torch.zeros(1, 4, 6, device=DEV)
    assert K.wgrad_first4(inp["w"], x6, (None, inp["dz"], inp["scale"], inp["shift"], inp["mean"], inp["invstd"],
                                         inp["coef"])) is None
    mom = torch.full((256 * 14,), float("nan"), dtype=torch.float64, device=DEV)
    with torch.cuda.device(DEV):
        assert int(lib.mlp_first4_moments(1, 8, None, mom.data_ptr(), K._stream(mom))) == INVALID
        assert int(lib.mlp_first4_moments(1, 8, inp["x"].data_ptr(), None, K._stream(mom))) == INVALID
        out = torch.full((4, 64), float("nan"), device=DEV)
        assert int(lib.mlp_first4_bn(mom.data_ptr(), 8.0, None, inp["gamma"].data_ptr(), inp["beta"].data_ptr(), 1e-5, 0.1,
                                     None, None, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                     out[3].data_ptr(), K._stream(mom))) == INVALID
        torch.cuda.synchronize()
    assert bool(torch.isnan(mom).all()) and bool(torch.isnan(out).all())
