"""SA1's 64 -> 128 Gram backward (csrc/mlp_pool_gram.hip: prep, the persistent pass, reduce, dw) against
the reference module's layer in float64 torch with autograd, at every form a workgroup's chunk range
takes for each nsample (tests/pool_gram128_cases.py has the table, tests/test_pool_gram128_cases.py
proves on the CPU what it covers and that the bound below fails a kernel with a bf16 term or a partial
product less).

Inputs: the statistics, arg-max, ymax and coef3 the backward consumes come from torch in float64,
rounded to fp32 (pool_gram128_cases.forward64) -- no forward kernel of the project takes part.  The
entry point is called through the library handle, so that every buffer it writes sits between guards
of the test's own, and once more through the Python wrapper.  Three rows (one per nsample) run a second
time with coef3's c1 = c2 = 0: the dense part is then zero and the truth is W3^T S and S a2^T, the
sparse LDS image alone.

Bound: per row and output, the kernel's relative L2 error and its max error over the range, both
against float64, stay within RATIO = 3 times what plain fp32 torch (two matmuls and the BatchNorm
algebra, pool_gram128_cases.plain_fp32) misses the same float64 values by on the same inputs, plus the
two floors of tests/test_pool_gram256_gpu.py, neither taken from the kernel's output: one fp32 ulp of
the largest element on the max error over the range, and on the two BatchNorm sums what one fp32 ulp
on every element of dq is worth in them (sums_resolution).  DESIGN.md has the measured table: no row
fails; dq uses at most 0.30 of its bound (0.52 sparse-only), dw 0.49; no figure needs the ulp floor; the
sums need theirs from T = 201 on (s_one 4.8e-6 at T = 4112 against 3 x 6.9e-7), at most 0.13 of it.  A
scratch build with the third bf16 term of the sparse entry forced to zero failed every row it was run
on (dq 9.5e-6 against a bound of 6.2e-7, inside the older caps).  The figures of
test_gpu_mlp.py::test_pooled_backward_from_the_gram_matrix stay as caps on top."""
import ctypes
import importlib

import pytest
import torch

from conftest import load_pkg
import pool_gram128_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096                  # floats on either side of every buffer the entry point writes
FILL = 0x7fc0dead             # a NaN no computation produces
INVALID = 1                   # hipErrorInvalidValue

# outer caps: (max over range, relative L2) of test_pooled_backward_from_the_gram_matrix
CAPS = {"dq": (3e-5, 2e-5), "dw": (1e-4, 1e-4)}
CAP_SUMS = 3e-6               # the sums against a float64 evaluation on the kernel's OWN dq, as there

RUNS = [c + (False,) for c in C.CASES] + [c + (True,) for c in C.CASES if c[:3] in C.SPARSE_ONLY]


def _K():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded(object):
    """n floats between two guards, the whole buffer one tensor filled with FILL"""

    def __init__(self, n, lead=0):
        self.raw = torch.full((GUARD + lead + n + GUARD,), FILL, dtype=torch.int32, device=DEV)
        self.lo, self.n = GUARD + lead, n
        self.view = self.raw[self.lo:self.lo + n].view(torch.float32)

    def guards_intact(self):
        return bool((self.raw[:self.lo] == FILL).all()) and bool((self.raw[self.lo + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.raw == FILL).all())


def _call(K, inp, fwd, dq, dw, sp, ws, y2=None, below_stats=True):
    """mlp_pool_gram_backward on the given buffers -> its return code"""
    b, r, ns = inp["b"], inp["r"], inp["ns"]
    y2 = inp["y2"] if y2 is None else y2
    p = K._grad_operand(pooled=(None, inp["dpooled"], fwd["argmax"], fwd["sc3"], fwd["sh3"], fwd["mean3"],
                                fwd["invstd3"], fwd["coef3"]), ns=ns)
    q = K._input_operand(y2, (fwd["sc2"], fwd["sh2"]), (fwd["mean2"], fwd["invstd2"]) if below_stats else None)
    with torch.cuda.device(y2.device):
        rc = K._lib.mlp_pool_gram_backward(b, C.M_OUT, C.K_IN, r, inp["w3"].data_ptr(), ctypes.byref(p),
                                           ctypes.byref(q), fwd["ymax"].data_ptr(), dq.data_ptr(), dw.data_ptr(),
                                           sp.data_ptr(), ws.data_ptr(), K._stream(y2))
        torch.cuda.synchronize()
    return int(rc)


def _buffers(b, r, parts, ws_floats, ws_lead=0):
    return (Guarded(b * C.K_IN * r), Guarded(C.M_OUT * C.K_IN), Guarded(C.K_IN * parts * 2),
            Guarded(ws_floats, lead=ws_lead))


@pytest.mark.parametrize("b,m,ns,seed", C.CASES)
def test_device_counts_are_the_mirrors(b, m, ns, seed):
    """The library's grid size and workspace are the mirror's for this device's CU count, and the ranges
    they give are those the table was laid out for: on a device with another count this fails, it does
    not quietly test other edges."""
    K = _K()
    cus, r = _cus(), m * ns
    assert int(K._lib.mlp_pool_gram_supported(b, C.M_OUT, C.K_IN, r, ns)) == 1 and C.covers(b, r, ns)
    assert int(K._lib.mlp_pool_gram_parts(b, C.M_OUT, C.K_IN, r)) == C.split(C.chunks(b, m, ns), C.LEAST, cus)[0]
    assert int(K._lib.mlp_pool_gram_workspace_floats(b, C.M_OUT, C.K_IN, r, ns)) == C.workspace_floats(b, m, ns, cus)
    assert C.describe(b, m, ns, cus) == C.describe(b, m, ns, C.CUS), \
        "%d CUs: the table of pool_gram128_cases.py was laid out for %d" % (cus, C.CUS)


@pytest.mark.parametrize("b,m,ns,seed,sparse_only", RUNS)
def test_gram128_backward_vs_float64(b, m, ns, seed, sparse_only):
    """Measured on an MI355X: DESIGN.md, "The Gram-128 backward against float64"."""
    K = _K()
    r, T, cus = m * ns, C.chunks(b, m, ns), _cus()
    inp = C.make_inputs(b, m, ns, seed, device=DEV)
    fwd = C.forward64(inp, sparse_only=sparse_only)
    info = C.check_inputs(inp, fwd)
    parts = int(K._lib.mlp_pool_gram_parts(b, C.M_OUT, C.K_IN, r))
    ws_floats = int(K._lib.mlp_pool_gram_workspace_floats(b, C.M_OUT, C.K_IN, r, ns))
    assert parts == C.split(T, C.LEAST, cus)[0] and ws_floats == C.workspace_floats(b, m, ns, cus)

    # ---- memory discipline: exactly the workspace asked for, guards round every written buffer
    dq, dw, sp, ws = _buffers(b, r, parts, ws_floats)
    assert all(t.view.data_ptr() % 16 == 0 for t in (dq, dw, sp, ws)) and inp["y2"].data_ptr() % 16 == 0
    assert _call(K, inp, fwd, dq.view, dw.view, sp.view, ws.view) == 0
    for name, t in (("dq", dq), ("dw", dw), ("stats_part", sp), ("workspace", ws)):
        assert t.guards_intact(), "%s: written outside the buffer" % name
    # no fill left: every element written, the zero partials of the empty workgroups included
    for name, t in (("dq", dq), ("dw", dw), ("stats_part", sp)):
        assert not bool((t.raw[t.lo:t.lo + t.n] == FILL).any()), "%s: an element never written" % name
        assert bool(torch.isfinite(t.view).all()), "%s: not finite" % name
    empty = C.describe(b, m, ns, cus)["empty"]
    if empty:
        assert bool((sp.view.view(C.K_IN, parts, 2)[:, parts - empty:] == 0).all())
    # the workspace 16 bytes further on (the double sums stay 8-byte aligned): the same bits
    dq2, dw2, sp2, ws2 = _buffers(b, r, parts, ws_floats, ws_lead=4)
    assert ws2.view.data_ptr() == ws2.raw.data_ptr() + 4 * (GUARD + 4) and ws2.view.data_ptr() % 16 == 0
    assert _call(K, inp, fwd, dq2.view, dw2.view, sp2.view, ws2.view) == 0
    for name, t in (("dq", dq2), ("dw", dw2), ("stats_part", sp2), ("workspace", ws2)):
        assert t.guards_intact(), "%s: written outside the buffer (second run)" % name
    # twice, and a third time through the wrapper: bit-equal (fixed ranges, fixed order of every sum)
    for first, second in ((dq, dq2), (dw, dw2), (sp, sp2)):
        assert torch.equal(first.view.view(torch.int32), second.view.view(torch.int32))
    del dq2, dw2, sp2, ws2, ws
    w_dq, w_dw, below = K.pool_gram_backward(inp["w3"], inp["y2"], (fwd["mean2"], fwd["invstd2"], fwd["sc2"], fwd["sh2"]),
                                             inp["g2"], fwd["coef3"], (fwd["mean3"], fwd["invstd3"], fwd["sc3"], fwd["sh3"]),
                                             inp["dpooled"], fwd["argmax"], fwd["ymax"], ns, True)
    assert torch.equal(w_dq.view(-1).view(torch.int32), dq.view.view(torch.int32))
    assert torch.equal(w_dw.view(-1).view(torch.int32), dw.view.view(torch.int32))
    del w_dq, w_dw

    # ---- numbers
    part = sp.view.view(C.K_IN, parts, 2).double()
    got = {"dq": dq.view.view(b, C.K_IN, r), "dw": dw.view.view(C.M_OUT, C.K_IN), "s_one": part[:, :, 0].sum(1),
           "s_xhat": part[:, :, 1].sum(1),
           # (the wrapper hands the coefficients back as the three rows of its scratch; in memory they are
           # the (64, 3) array the kernels read: column 0 is every third float)
           "coef0": below[2].contiguous().view(-1)[0::3]}
    # the wrapper's finalize hands on the same sums (dgamma, dbeta of the layer below)
    for mine, theirs in ((got["s_xhat"], below[0]), (got["s_one"], below[1])):
        assert float((theirs.double() - mine).abs().max()) <= 2e-7 * float(mine.abs().max())
    ref = C.reference64(inp, fwd)
    p32 = C.plain_fp32(inp, fwd)
    resolution = C.sums_resolution(inp, fwd, ref)
    tag = "gram128%s (%d, %d, %d) T %d shut %.3f" % (" sparse-only" if sparse_only else "", b, m, ns, T, info["shut"])
    bad = []
    for name in C.OUTPUTS:
        e, e32 = C.errors(got[name], ref[name]), C.errors(p32[name], ref[name])
        ok, bound = C.within(name, e, e32, resolution)
        alone = e[0] <= C.RATIO * e32[0] and e[1] <= C.RATIO * e32[1]
        print("%s %-6s kernel rel-L2 %.2e max/range %.2e | fp32 torch %.2e %.2e | bound %.2e %.2e | %s"
              % (tag, name, e[0], e[1], e32[0], e32[1], bound[0], bound[1],
                 "MISSES the bound" if not ok else "within 3 x fp32 alone" if alone else "needs the floor"))
        if not ok:
            bad.append((name, e, e32, bound))
        if name in CAPS and not (e[1] <= CAPS[name][0] and e[0] <= CAPS[name][1]):
            bad.append((name, "cap", e))
    # the sums against float64 sums over the kernel's own dq (the cap of the older test)
    y2 = inp["y2"].double().view(b, C.K_IN, r)
    gate = (y2 * fwd["sc2"].double().view(1, -1, 1) + fwd["sh2"].double().view(1, -1, 1)) > 0
    gd = torch.where(gate, got["dq"].double(), torch.zeros((), dtype=torch.float64, device=DEV))
    xh = (y2 - fwd["mean2"].double().view(1, -1, 1)) * fwd["invstd2"].double().view(1, -1, 1)
    own = (C.errors(got["s_xhat"], (gd * xh).sum(dim=(0, 2)))[0], C.errors(got["s_one"], gd.sum(dim=(0, 2)))[0])
    print("%s sums against float64 sums of the kernel's own dq: %.2e %.2e" % ((tag,) + own))
    if max(own) > CAP_SUMS:
        bad.append(("sums of own dq", own))
    assert not bad, bad


def _refusal(K, b, m, ns, *, ws_shift=0, y2_shift=0, below_stats=True):
    inp = C.make_inputs(b, m, ns, 0, device=DEV)
    fwd = C.forward64(inp)
    r = m * ns
    # (buffers as large as any reading of the shape could want: a call that ran after all stays inside)
    assert C.split(4112, C.LEAST, _cus())[0] == _cus()   # (the workspace of a grid at the CU count)
    dq, dw, sp, ws = _buffers(b, r, _cus(), C.workspace_floats(2, 2056, 32, _cus()) + 4 * C.SUMS, ws_lead=ws_shift)
    y2 = inp["y2"]
    if y2_shift:
        hold = torch.zeros(y2.numel() + 8, device=DEV)
        y2 = hold[y2_shift:y2_shift + y2.numel()].view_as(inp["y2"]).copy_(inp["y2"])
        assert y2.data_ptr() % 16 != 0 and y2.is_contiguous()
    if ws_shift:
        assert ws.view.data_ptr() % 16 != 0
    rc = _call(K, inp, fwd, dq.view, dw.view, sp.view, ws.view, y2=y2, below_stats=below_stats)
    assert rc == INVALID, rc
    for name, t in (("dq", dq), ("dw", dw), ("stats_part", sp), ("workspace", ws)):
        assert t.untouched(), "%s written by a refused call" % name


@pytest.mark.parametrize("what,b,m,ns,how", [
    ("T = 63", 1, 63, 32, {}), ("ns = 8", 1, 256, 8, {}), ("ns = 128", 1, 16, 128, {}),
    ("r % 32 != 0", 1, 129, 16, {}),
    ("workspace not 16-byte aligned", 1, 64, 32, {"ws_shift": 1}),
    ("y2 not 16-byte aligned", 1, 64, 32, {"y2_shift": 1}),
    ("the layer below without mean / invstd", 1, 64, 32, {"below_stats": False})])
def test_gram128_refusals(what, b, m, ns, how):
    """hipErrorInvalidValue, nothing launched: every output still holds its fill pattern"""
    K = _K()
    r = m * ns
    # the refusal is the one the row names: the shape is otherwise in order
    assert int(K._lib.mlp_pool_gram_supported(b, C.M_OUT, C.K_IN, r, ns)) == (1 if how else 0)
    assert C.covers(b, r, ns) == bool(how)
    _refusal(K, b, m, ns, **how)
