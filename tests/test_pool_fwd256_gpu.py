"""The pooled 128 -> 256 forward (csrc/mlp_pool_fwd256.hip: pool_fwd256_kernel<16|32, STORE>) and the tiled
kernel behind the same entry point (gemm_nn2_kernel with its pooled epilogue) against the reference module's
layer in float64 torch, at every form a workgroup's block range takes in the persistent kernel
(tests/pool_fwd256_cases.py has the table, tests/test_pool_fwd256_cases.py proves on the CPU what it covers).

The entry point mlp_gemm_forward_stats_pool is called through the library handle, so that every buffer it
writes (pairs, the two ext planes, y) sits between NaN-filled guards of the test's own.  No kernel of the
project prepares an input.

Exact, per row: the two forms (with and without the store of y) leave the same bits; ext names the FIRST
extreme of the kernel's own stored y in every group and channel; a planted later copy never wins; the constant
channel is 0 with index 0 and pairs (0, 0); a refused call writes nothing.

Bounds: e(kernel) <= RATIO * e(plain fp32) + floor (sa1_train_cases.within, RATIO = 3), each figure against
float64.  Floors, none taken from the kernel's output: for y and the winners one fp32 ulp of the range
(tensor_floors); for the per-tile pairs what one ulp on every element of y is worth in them (pair_floors);
for the pairs against float64 statistics of the kernel's OWN stored y one ulp of each output
(own_pair_floors), the yardstick there being fp32 two-pass statistics of that same y.

Measured on an MI355X (256 CUs), worst row of the twelve; need = e(kernel) / bound.  kernel / plain fp32:
  measure                     pool_fwd256_kernel                          tiled kernel (five small rows, ns 64)
  y, max / range              3.7-7.0e-7 / 5.0-8.8e-7, need 0.28 (37,112,16)   4.9-8.4e-7 / 5.0-7.8e-7, need 0.41
  y, worst channel / sigma    1.9-4.2e-5 / 2.6-5.2e-5, need 0.29 (1,2064,16)   2.6-4.9e-5 / 2.6-4.6e-5, need 0.41
  winner, max / range         2.8-6.2e-7 / 3.2-7.3e-7, need 0.30 (257,8,32)    2.6-6.2e-7 / 3.2-6.1e-7, need 0.38
  winner index outside the excluded pairs: equal to the truth's in every row, both kernels
  tile mean / sigma           3.3-8.9e-6 / 3.1e-6-1.0e-5, need 0.27 (3,16,16)  2.4e-6-1.2e-5 / 3.1-9.1e-6, need 0.48
  tile M2 / (64 var)          2.6e-6-1.0e-5 / 2.9e-6-1.0e-5, need 0.24         3.6-9.3e-6 / 2.9-7.9e-6, need 0.34
  own y: tile mean            2.9-6.2e-6 / 2.3-8.7e-6, need 0.24               2.1-6.2e-6 / 3.4-7.4e-6, need 0.30
  own y: tile M2              8.3e-7-3.9e-6 / 1.4-2.6e-7, need 0.12 (5,1232,16) 1.4-3.5e-6 / 1.4-1.9e-7, need 0.09
  finalize kernel vs formula  mean 0.19, invstd 0.12, scale 0.17, shift 0.39   0.16, 0.11, 0.20, 0.27
  batch statistics vs truth   mean 0.25, invstd 0.14, scale 0.19, shift 0.14   0.25, 0.25, 0.25, 0.22
The worst-channel figures are those of OFFSET_ROWS (40-58 sigma from zero), where plain fp32 sits too.
"own y: tile M2" is the one figure that one ulp of the output does not cover: the kernels' one-pass shifted
sums miss the float64 M2 of their own y by up to 3.9e-6 where two-pass fp32 misses it by 2.6e-7 (need up to
4.8 with one ulp of M2 as the only floor, in every row and in both kernels alike).  The floor added for it
is the first-order rounding bound of those sums from the fp32 format (pool_fwd256_cases.one_pass_floor), not
a figure of the kernel's: the kernels need 0.12 of it at most.
The stored y against the six-product form of the operands' bf16 terms in float64: no closer than to the
truth (max / range 3.6-7.0e-7 to the form, 3.7-7.0e-7 to the truth; the form itself is 3-6e-8 from the
truth): what the kernel misses is the fp32 accumulator's roundings over 48 chained MFMAs, not the three
dropped products.  A NaN column of y2 reaches the product as 0 (0 of the group's y3 are NaNs); +inf does
reach the pool as NaNs.
Mutants of mlp_pool_fwd256.hip, each run once against this file and against
test_gpu_mlp.py::test_pooled_forward_without_its_raw_output (scratch builds, not kept):
  the cloud of a chunk taken from the range's first chunk    5 rows fail here (every crossing row: an ext element
                                                             never written); the older test fails 1 case of 8
                                                             ((12, 1024, 32): per = 12 does cross at 256 CUs)
  lower half-wave preferred on equal values (piece 18)       17 fail here (the later copy of pair (5, 8) wins);
                                                             the older test passes
  lower register half scanned before the upper               19 fail here (pair (2, ns / 2 + 1)); the older passes
  PF_MM1(hi, lo) replaced by (lo, lo)                        12 fail here (y at need 2.8-4.5); the older fails
  the 16 dlt dlt term dropped                                12 fail here (tile M2 at need 8800-31000); the older fails
"""
import ctypes
import importlib

import pytest
import torch

from conftest import load_pkg
import pool_fwd256_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096                  # floats on either side of every buffer the entry point writes
FILL = 0x7fc0dead             # a NaN no computation produces
INVALID = 1                   # hipErrorInvalidValue
ROWS = [c[:3] for c in C.CASES]
PER1 = tuple(c for c in C.CASES if C.describe(*c[:3])["per"] == 1)
SHARED_COLS = 16384           # rows up to this many columns keep their reference for the other tests


def _K():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


@pytest.fixture(autouse=True)
def _pooled_path(monkeypatch):
    """the small rows take the pooled path too (the library reads both variables on every call)"""
    monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "0")
    monkeypatch.delenv("MLP_POOL_FWD256", raising=False)


class Guarded(object):
    """n floats between two guards, the whole buffer one tensor filled with FILL"""

    def __init__(self, n, lead=0):
        self.raw = torch.full((GUARD + lead + n + GUARD,), FILL, dtype=torch.int32, device=DEV)
        self.lo, self.n = GUARD + lead, n
        self.view = self.raw[self.lo:self.lo + n].view(torch.float32)

    def guards_intact(self):
        return bool((self.raw[:self.lo] == FILL).all()) and bool((self.raw[self.lo + self.n:] == FILL).all())

    def all_written(self):
        return not bool((self.raw[self.lo:self.lo + self.n] == FILL).any())

    def untouched(self):
        return bool((self.raw == FILL).all())


_SHARED = {}


def _reference(b, groups, ns, seed):
    """(inp, tru, p32, info) on the device, computed once for the small rows and left unchanged"""
    key = (b, groups, ns, seed)
    if key in _SHARED:
        return _SHARED[key]
    inp = C.make_inputs(b, groups, ns, seed, device=DEV)
    tru = C.truth64(inp)
    info = C.check_inputs(inp, tru)
    out = (inp, tru, C.plain_fp32(inp), info)
    if b * groups * ns <= SHARED_COLS:
        _SHARED[key] = out
    return out


def _buffers(b, groups, ns, y_lead=0, store=True):
    r = groups * ns
    return {"pairs": Guarded(b * (r // C.TILE) * C.M_OUT * 2), "ext": Guarded(2 * b * C.M_OUT * groups),
            "y": Guarded(b * C.M_OUT * r, lead=y_lead) if store else None}


def _call(K, inp, buf, *, y2=None, w=None, null=(), shape=None):
    """mlp_gemm_forward_stats_pool on the given buffers -> its return code"""
    b, r, ns = shape if shape else (inp["b"], inp["r"], inp["ns"])
    y2 = inp["y2"] if y2 is None else y2
    w = inp["w3"] if w is None else w
    op = K._input_operand(y2, (inp["scale"], inp["shift"]))
    ptr = lambda name, t: None if (name in null or t is None) else t.data_ptr()  # noqa: E731
    with torch.cuda.device(y2.device):
        rc = K._lib.mlp_gemm_forward_stats_pool(b, C.M_OUT, C.K_IN, r, w.data_ptr(), ctypes.byref(op),
                                                ptr("y", buf["y"].view if buf["y"] else None),
                                                ptr("pairs", buf["pairs"].view), ns, ptr("gamma", inp["gamma3"]),
                                                ptr("ext", buf["ext"].view), K._stream(y2))
        torch.cuda.synchronize()
    return int(rc)


def _views(inp, buf):
    b, groups, ns = inp["b"], inp["groups"], inp["ns"]
    ext = buf["ext"].view.view(2, b, C.M_OUT, groups)
    return {"pairs": buf["pairs"].view.view(-1, C.M_OUT, 2), "win": ext[0], "idx": ext[1].view(torch.int32),
            "y": buf["y"].view.view(b, C.M_OUT, groups, ns) if buf["y"] else None}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(K, inp, store=True, y_lead=0, **kw):
    """one call on fresh guarded buffers: return code 0, guards intact, every element written -> views"""
    buf = _buffers(inp["b"], inp["groups"], inp["ns"], y_lead=y_lead, store=store)
    assert _call(K, inp, buf, **kw) == 0
    for name, t in buf.items():
        if t is not None:
            assert t.guards_intact(), "%s: written outside the buffer" % name
            assert t.all_written(), "%s: an element never written" % name
    got = _views(inp, buf)
    got["buf"] = buf
    return got


def _exact(inp, got, label):
    """what holds without a tolerance, on the kernel's own output"""
    ns, groups = inp["ns"], inp["groups"]
    idx, win, y = got["idx"], got["win"], got["y"]
    # (first: a later gather uses these indices)
    assert int(idx.min()) >= 0 and int(idx.max()) < ns, "%s: an index outside [0, ns)" % label
    for cls, (_, later) in enumerate(C.tie_pairs(ns)):
        assert not bool((idx[:, :, cls::4] == later).any()), "%s: the later copy of pair %d won" % (label, cls)
    assert bool((idx[:, C.ZERO_ROW] == 0).all()) and bool((_bits(win[:, C.ZERO_ROW]) == 0).all()), label
    assert bool((_bits(got["pairs"][:, C.ZERO_ROW]) == 0).all()), "%s: the constant channel's pairs" % label
    if y is None:
        return
    assert bool((_bits(y[:, C.ZERO_ROW]) == 0).all()), label
    picked = torch.gather(y, 3, idx.long().unsqueeze(-1)).squeeze(-1)
    assert torch.equal(_bits(picked), _bits(win)), "%s: ext[0] is not the stored y at ext[1]" % label
    v, first = C.first_winner(y, inp["gamma3"])
    assert torch.equal(first.int(), idx), "%s: ext[1] is not the FIRST extreme of the stored y" % label
    assert torch.equal(v * C.pool_sign(inp["gamma3"]).view(1, -1, 1), win), label


def _rule(rows, name, e, e32, floor):
    ok, need, worst, worst32 = C.within(e, e32, floor)
    rows.append((name, bool(ok), float(need), float(worst), float(worst32)))


def _numbers(K, inp, tru, p32, info, got, label, layout="t"):
    """every measure of one run under the rule -> list of (name, ok, need, e, e32); printed before asserted"""
    rows = []
    st = tru["stats"]
    var = st["var"]
    y = got["y"]
    if y is not None:
        (eg, ec), (pg, pc) = C.tensor_errors(y, tru["y3"], var), C.tensor_errors(p32["y3"], tru["y3"], var)
        fg, fc = C.tensor_floors(tru["y3"], var)
        _rule(rows, "y global", eg, pg, fg)
        _rule(rows, "y channel", ec, pc, fc)
    (eg, ec), (pg, pc) = C.tensor_errors(got["win"], tru["win"], var), C.tensor_errors(p32["win"], tru["win"], var)
    fg, fc = C.tensor_floors(tru["win"], var)
    _rule(rows, "winner global", eg, pg, fg)
    _rule(rows, "winner channel", ec, pc, fc)
    # the winners' indices, outside the (group, channel) pairs whose rival is within WIN_ULPS of them
    differ = (got["idx"] != tru["idx"].int()) & ~info["near"]
    rows.append(("index", not bool(differ.any()), float(differ.sum()), float(differ.sum()), 0.0))
    # the per-tile pairs against the truth's
    e, e32, fl = C.pair_errors(got["pairs"], tru["pairs"], var), C.pair_errors(p32["pairs"], tru["pairs"], var), \
        C.pair_floors(tru["y3"], var)
    _rule(rows, "tile mean", e[0], e32[0], fl[0])
    _rule(rows, "tile M2", e[1], e32[1], fl[1])
    if y is not None:
        # more sharply: against float64 statistics of the kernel's own stored y (both sides read the same y:
        # the matrix pipe's one-sided rounding does not enter)
        want = C.tile_pairs(y.double())
        e, e32, fl = C.pair_errors(got["pairs"], want, var), C.pair_errors(C.tile_pairs(y), want, var), \
            C.own_pair_floors(want, var)
        _rule(rows, "own tile mean", e[0], e32[0], fl[0])
        _rule(rows, "own tile M2", e[1], e32[1], fl[1] + C.one_pass_floor(tru["y3"], var, layout))
        del want
    # the finalize kernel on these pairs against the formula in float64 on them, and both against the truth
    parts = got["pairs"].shape[0]
    gamma, beta = inp["gamma3"], inp["beta3"]
    f64 = C.finalize64(got["pairs"], C.TILE, gamma, beta, inp["eps"], inp["momentum"])
    f64.update(gamma=gamma, beta=beta, eps=inp["eps"])
    with torch.cuda.device(got["pairs"].device):
        kern = K._finalize_pairs(C.M_OUT, parts, C.TILE, got["pairs"].contiguous(), gamma, beta, None, None,
                                 inp["momentum"], inp["eps"])
        torch.cuda.synchronize()
    e, e32, fl = C.stat_errors(kern, f64), C.stat_errors(C.finalize_fp32(got["pairs"], C.TILE, gamma, beta, inp["eps"]), f64), \
        C.own_floors(f64)
    for k in ("mean", "invstd", "scale", "shift"):
        _rule(rows, "finalize " + k, e[k], e32[k], fl[k])
    tup = lambda s: (s["mean"], s["invstd"], s["scale"], s["shift"])  # noqa: E731
    e32, fl = C.stat_errors(tup(p32["stats"]), st), C.stat_floors(tru["y3"], st)
    for who, stats in (("batch", kern), ("batch64", tup(f64))):
        e = C.stat_errors(stats, st)
        for k in ("mean", "invstd", "scale", "shift"):
            _rule(rows, "%s %s" % (who, k), e[k], e32[k], fl[k])
    for name, ok, need, e, e32 in rows:
        print("fwd256 %-34s %-16s need %.3f kernel %.3e plain fp32 %.3e%s" % (label, name, need, e, e32, "" if ok else "  <-- FAILS"))
    return rows


def _split_form(inp, tru, y, label):
    """how much closer the stored y is to the six-product form than to the truth (recorded, not asserted:
    the form leaves the accumulator's roundings out)"""
    own = C.split_form64(inp)
    rng = float(tru["y3"].abs().max())
    d_form, d_truth = float((y.double() - own).abs().max()) / rng, float((y.double() - tru["y3"]).abs().max()) / rng
    form_truth = float((own - tru["y3"]).abs().max()) / rng
    print("fwd256 %-34s max/range: y - six-product form %.3e, y - truth %.3e, form - truth %.3e" % (label, d_form, d_truth, form_truth))
    return d_form, d_truth


def test_device_reaches_every_edge():
    """The table was laid out for 256 CUs: on a device with another count this fails, it does not quietly test
    other edges."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reached = C.edges(ROWS, cus)
    assert reached >= C.EDGES, "%d CUs: the table of pool_fwd256_cases.py misses %s" % (cus, sorted(C.EDGES - reached))


@pytest.mark.parametrize("b,groups,ns,seed", C.CASES)
def test_pool_fwd256_vs_float64(b, groups, ns, seed):
    K = _K()
    inp, tru, p32, info = _reference(b, groups, ns, seed)
    assert C.covers(b, C.M_OUT, C.K_IN, groups * ns, ns) and inp["w3"].data_ptr() % 16 == 0 and inp["y2"].data_ptr() % 16 == 0
    label = "(%d, %d, %d)" % (b, groups, ns)
    stored = _run(K, inp, store=True)
    assert stored["y"].data_ptr() % 16 == 0
    bare = _run(K, inp, store=False)
    # the two forms: the same accumulators, the same bits
    assert torch.equal(_bits(stored["pairs"]), _bits(bare["pairs"])), "pairs differ between the two forms"
    assert torch.equal(_bits(stored["win"]), _bits(bare["win"])) and torch.equal(stored["idx"], bare["idx"])
    _exact(inp, stored, label)
    _exact(inp, bare, label + " no y")
    rows = _numbers(K, inp, tru, p32, info, stored, label)
    _split_form(inp, tru, stored["y"], label)
    bad = [row for row in rows if not row[1]]
    assert not bad, bad


@pytest.mark.parametrize("b,groups,ns,seed", PER1 + (C.TILED_EXTRA,))
def test_tiled_kernel_behind_the_same_entry(b, groups, ns, seed, monkeypatch):
    """MLP_POOL_FWD256=0 (and nsample 64 in any case): gemm_nn2_kernel<256, 64, 4, 1> with its pooled epilogue"""
    K = _K()
    inp, tru, p32, info = _reference(b, groups, ns, seed)
    label = "(%d, %d, %d) tiled" % (b, groups, ns)
    mine = _run(K, inp, store=True) if ns != 64 else None
    monkeypatch.setenv("MLP_POOL_FWD256", "0")
    stored = _run(K, inp, store=True)
    bare = _run(K, inp, store=False)
    assert torch.equal(_bits(stored["pairs"]), _bits(bare["pairs"])), "pairs differ between the two forms"
    assert torch.equal(_bits(stored["win"]), _bits(bare["win"])) and torch.equal(stored["idx"], bare["idx"])
    _exact(inp, stored, label)
    _exact(inp, bare, label + " no y")
    rows = _numbers(K, inp, tru, p32, info, stored, label, layout="tiled")
    bad = [row for row in rows if not row[1]]
    if mine is not None:
        # the two kernels: their index planes may differ only where a rival is within WIN_ULPS of the winner
        differ = (mine["idx"] != stored["idx"]) & ~info["near"]
        assert not bool(differ.any()), int(differ.sum())
    assert not bad, bad


@pytest.mark.parametrize("value", ["nan", "inf"])
@pytest.mark.parametrize("b,groups,ns,seed", [c for c in C.CASES if c[:2] in ((3, 8), (3, 16))])
def test_group_of_nans(b, groups, ns, seed, value):
    """One group of cloud 1 whose every column is NaN in every input channel.  The input layer's ReLU is a
    maximum with 0, which returns 0 for a NaN: such a group reaches the product as zeros and the pool as a tie
    of all its samples.  +inf survives the ReLU (channels with a positive scale) and splits into (inf, NaN,
    NaN): every y3 of the group is a NaN, nothing compares, and the `aa == 64` branch sets the index.  In both
    the index is 0 and in range, and nothing outside the group's tile changes by a bit."""
    K = _K()
    inp = _reference(b, groups, ns, seed)[0]
    cloud, grp = 1, 5
    bad = dict(inp)
    bad["y2"] = inp["y2"].clone()
    bad["y2"][cloud, :, grp, :] = float(value)
    clean, got = _run(K, inp, store=True), _run(K, bad, store=True)
    idx = got["idx"]
    assert int(idx.min()) >= 0 and int(idx.max()) < ns   # before anything is gathered with it
    assert bool((idx[cloud, :, grp] == 0).all())
    if value == "inf":
        assert bool(torch.isnan(got["y"][cloud, :, grp]).all())   # the group did reach the pool as NaNs
    else:
        print("fwd256 (%d, %d, %d) NaN group: y3 of the group NaN in %d of %d elements" %
              (b, groups, ns, int(torch.isnan(got["y"][cloud, :, grp]).sum()), C.M_OUT * ns))
    per_cloud = groups * ns // C.TILE
    tiles = sorted({cloud * per_cloud + col // C.TILE for col in range(grp * ns, (grp + 1) * ns)})
    keep = torch.ones(b * per_cloud, dtype=torch.bool, device=DEV)
    keep[tiles] = False
    assert torch.equal(_bits(got["pairs"][keep]), _bits(clean["pairs"][keep]))
    keep = torch.ones(b, groups, dtype=torch.bool, device=DEV)
    keep[cloud, grp] = False
    for name in ("win", "idx", "y"):
        a, c = (t.transpose(1, 2)[keep] for t in (got[name], clean[name]))   # (b, groups, 256[, ns])
        assert torch.equal(_bits(a), _bits(c)), "%s changed outside the group" % name
    # the kernel that does not store y agrees on the indices
    assert torch.equal(_run(K, bad, store=False)["idx"], idx)


def _declined(K, inp, **kw):
    b, groups, ns = inp["b"], inp["groups"], inp["ns"]
    # (buffers as large as any reading of the shape could want: a call that ran after all stays inside)
    buf = _buffers(b, 2 * groups, ns)
    rc = _call(K, inp, buf, **kw)
    assert rc == INVALID, rc
    for name, t in buf.items():
        assert t.untouched(), "%s written by a refused call" % name


@pytest.mark.parametrize("what", ["pairs", "ext", "gamma", "w off 16 bytes", "r % 256 != 0"])
@pytest.mark.parametrize("b,groups,ns,seed", C.CASES[:2])
def test_declines(b, groups, ns, seed, what):
    """hipErrorInvalidValue, nothing launched: every output still holds its fill pattern"""
    K = _K()
    inp = _reference(b, groups, ns, seed)[0]
    if what in ("pairs", "ext", "gamma"):
        _declined(K, inp, null=(what,))
    elif what == "w off 16 bytes":
        hold = torch.zeros(C.M_OUT * C.K_IN + 8, device=DEV)
        w = hold[1:1 + C.M_OUT * C.K_IN].view(C.M_OUT, C.K_IN).copy_(inp["w3"])
        assert w.data_ptr() % 16 == 4 and w.is_contiguous()
        _declined(K, inp, w=w)
    else:
        r = groups * ns // 2   # 128 columns: the statistics epilogue does not cover them
        assert r % 256 != 0 and not K._lib.mlp_gemm_forward_stats_pool_supported(b, C.M_OUT, C.K_IN, r, ns)
        _declined(K, inp, shape=(b, r, ns))


@pytest.mark.parametrize("b,groups,ns,seed", C.CASES[2:4])
def test_y_off_16_bytes_is_served_by_the_tiled_kernel(b, groups, ns, seed, monkeypatch):
    K = _K()
    inp, tru, p32, info = _reference(b, groups, ns, seed)
    label = "(%d, %d, %d) y + 4 bytes" % (b, groups, ns)
    got = _run(K, inp, store=True, y_lead=1)
    assert got["y"].data_ptr() % 16 == 4
    _exact(inp, got, label)
    rows = _numbers(K, inp, tru, p32, info, got, label, layout="tiled")
    bad = [row for row in rows if not row[1]]
    assert not bad, bad
    monkeypatch.setenv("MLP_POOL_FWD256", "0")
    tiled = _run(K, inp, store=True)
    for name in ("pairs", "win", "idx", "y"):
        assert torch.equal(_bits(got[name]), _bits(tiled[name])), name
