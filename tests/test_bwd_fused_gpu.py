"""The one-pass layer backward (csrc/mlp_bwd_fused.hip: gemm_bwd_fused_kernel) in each of its seven
instantiations against float64, at every form a workgroup's chunk range takes (tests/bwd_fused_cases.py
has the forms and the tables, tests/test_bwd_fused_cases.py proves on the CPU what they cover).

Inputs: everything the backward consumes -- the raw output, both layers' statistics and folded (scale,
shift), arg-max, coef -- comes from torch in float64, rounded to fp32 (bwd_fused_cases.forward64); no
kernel of the project takes part.  The entry point is called through the library handle, as
tests/test_bwd_x6_roles.py does, so that dq, dw, stats_part and the workspace (exactly as large as the
library asks for) each sit between NaN-pattern guards; twice, bit-equal; and once through the wrapper.

Bound, per case and output: outer caps from the project (tests/test_gpu_mlp.py::
test_fused_backward_vs_two_gemms: 1e-5 dx, 2e-5 dw, 2e-5 the sums and coef), here against the truth's
own range; inside them the kernel's relative L2 error and its max error over the range stay within
RATIO = 3 times what plain fp32 torch (bwd_fused_cases.plain_fp32) misses the same float64 values by on
the same inputs.  Two floors, neither from the kernel's output: one fp32 ulp of the largest element on
the max error, and for everything summed over dx (the two sums, the coefficient columns built from
them, LIN4's G and dw0) what one ulp on every element of dx is worth in it (bwd_fused_cases.resolution;
measured need at most 0.07 of it).  One form needs a third: dw of pooled (128,64) is 1.3-1.7e-6 off at
T = 64 ... 89 where plain fp32 is 3.7-6.4e-7 off, 5.1e-6 against 1.1e-6 at T = 2057 -- the matrix pipe
cuts the thousands of small one-signed products of a pooled operand's dense half toward zero
(bwd_fused_cases.DW_FLOOR says how that was found); its floor is one ulp on every term of the dot
product, ULP sum |P Q|, measured need at most 0.70 of it.  DESIGN.md has the reasoning and the table of
every row's figures."""
import ctypes
import importlib

import pytest
import torch

from conftest import load_pkg
import bwd_fused_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096                  # floats on either side of every buffer the entry point writes
FILL = 0x7fc0dead             # a NaN no computation produces
CAPS = {"dx": 1e-5, "xyz": 1e-5, "dw": 2e-5, "s_one": 2e-5, "s_xhat": 2e-5, "coef0": 2e-5, "coef1": 2e-5,
        "coef2": 2e-5, "G": 2e-5, "dw0": 2e-5, "dgamma": 2e-5, "dbeta": 2e-5}
ROWS = [(f,) + c for f in C.FORMS for c in C.CASES[f]]


def _K():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded(object):
    """n floats between two guards, the whole buffer one tensor filled with FILL"""

    def __init__(self, n):
        self.raw = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.int32, device=DEV)
        self.n = n
        self.view = self.raw[GUARD:GUARD + n].view(torch.float32)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == FILL).all()) and bool((self.raw[GUARD + self.n:] == FILL).all())

    def all_written(self):
        return not bool((self.raw[GUARD:GUARD + self.n] == FILL).any())


def _operands(K, form, inp, fwd):
    m, k, pmode, qmode, _, _ = C.FORMS[form]
    rec = (fwd["sc"], fwd["sh"], fwd["mean"], fwd["invstd"], fwd["coef"])
    if pmode == C.OP_POOLDY:
        kw = dict(pooled=(fwd["y"], inp["dz"], fwd["argmax"]) + rec)
    else:
        kw = dict(fly=(fwd["y"], inp["dz"]) + rec)
    if qmode == C.OP_DIRECT:
        return kw, dict(x=inp["x"])
    xkw = dict(x=inp["x4"] if qmode == C.OP_LIN4 else inp["x"], xcoeff=(fwd["scx"], fwd["shx"]),
               xstats=(fwd["meanx"], fwd["invx"], inp["gx"], True))
    if qmode == C.OP_LIN4:
        xkw["lin_w"] = inp["w0"]
    return kw, xkw


def _direct(K, form, inp, fwd, parts, ws_floats):
    """mlp_gemm_backward_fused on guarded buffers of the test's own -> (dq, dw, sp, ws), dq / sp None
    where the form has none"""
    m, k, pmode, qmode, dgrad, sums = C.FORMS[form]
    b, r = inp["b"], inp["r"]
    kw, xkw = _operands(K, form, inp, fwd)
    p = K._grad_operand(**kw)
    q = K._input_operand(xkw["x"], xkw.get("xcoeff"), xkw.get("xstats"), xkw.get("lin_w"))
    assert (p.mode, q.mode) == (pmode, qmode)
    assert K._lib.mlp_gemm_backward_fused_supported(b, m, k, r, p.mode, q.mode, p.ns) == 1
    dq = Guarded(parts * 64 * 4) if qmode == C.OP_LIN4 else (Guarded(b * k * r) if dgrad else None)
    dw, ws = Guarded(m * k), Guarded(ws_floats)
    sp = Guarded(k * parts * 2) if sums else None
    for t in (dq, dw, ws, sp):
        assert t is None or t.view.data_ptr() % 16 == 0
    with torch.cuda.device(inp["w"].device):
        rc = K._lib.mlp_gemm_backward_fused(b, m, k, r, inp["w"].data_ptr(), ctypes.byref(p), ctypes.byref(q),
                                            dq.view.data_ptr() if dq is not None else None, dw.view.data_ptr(),
                                            ws.view.data_ptr(), sp.view.data_ptr() if sp is not None else None,
                                            K._stream(inp["w"]))
        torch.cuda.synchronize()
    assert int(rc) == 0, rc
    for name, t in (("dq", dq), ("dw", dw), ("stats_part", sp), ("workspace", ws)):
        if t is not None:
            assert t.guards_intact(), "%s: written outside the buffer" % name
            # (the workspace too: every workgroup, an empty one as well, leaves a whole weight partial)
            assert t.all_written(), "%s: an element never written" % name
            assert name == "workspace" or not bool(torch.isnan(t.view).any()), "%s: NaN" % name
    return dq, dw, sp, ws


def _moments(x4):
    """mlp_first4_moments' layout from float64 torch: 256 partial rows of 14 doubles (4 sums, the 10
    products of the upper triangle), here the totals in row 0"""
    b, r = x4.shape[0], x4.shape[2] * x4.shape[3]
    x = x4.double().view(b, 4, r)
    s = torch.einsum("bcr,bdr->cd", x, x)
    row = [x[:, c].sum() for c in range(4)] + [s[c, d] for c in range(4) for d in range(c, 4)]
    mom = torch.zeros(256, 14, dtype=torch.float64, device=x4.device)
    mom[0] = torch.stack(row)
    return mom.view(-1).contiguous()


@pytest.mark.parametrize("form,b,groups,ns,seed", ROWS)
def test_device_counts_are_the_mirrors(form, b, groups, ns, seed):
    """The library's grid shows in stats_parts and workspace_floats: they are the mirror's for this
    device's CU count, and the ranges are those the table was laid out for -- on a device with another
    count this fails, it does not quietly test other edges."""
    K = _K()
    m, k = C.FORMS[form][:2]
    cus, r = _cus(), groups * ns
    assert int(K._lib.mlp_gemm_backward_fused_stats_parts(b, m, k, r)) == C.stats_parts(b, m, k, r, cus)
    assert int(K._lib.mlp_gemm_backward_fused_workspace_floats(b, m, k, r)) == C.workspace_floats(b, m, k, r, cus)
    assert C.describe(form, b, groups, ns, cus) == C.describe(form, b, groups, ns, C.CUS), \
        "%d CUs: the tables of bwd_fused_cases.py were laid out for %d" % (cus, C.CUS)


@pytest.mark.parametrize("form,b,groups,ns,seed", ROWS)
def test_fused_backward_vs_float64(form, b, groups, ns, seed):
    K = _K()
    m, k, pmode, qmode, dgrad, sums = C.FORMS[form]
    r, cus = groups * ns, _cus()
    d = C.describe(form, b, groups, ns, cus)
    inp = C.make_inputs(form, b, groups, ns, seed, device=DEV)
    fwd = C.forward64(form, inp)
    info = C.check_inputs(form, inp, fwd)
    parts = int(K._lib.mlp_gemm_backward_fused_stats_parts(b, m, k, r))
    ws_floats = int(K._lib.mlp_gemm_backward_fused_workspace_floats(b, m, k, r))
    assert parts == C.stats_parts(b, m, k, r, cus) == (2 * d["g"] if sums else 0)
    assert ws_floats == C.workspace_floats(b, m, k, r, cus) == d["g"] * m * k

    # ---- memory discipline, twice, bit-equal
    dq, dw, sp, ws = _direct(K, form, inp, fwd, parts, ws_floats)
    dq2, dw2, sp2, ws2 = _direct(K, form, inp, fwd, parts, ws_floats)
    for first, second in ((dq, dq2), (dw, dw2), (sp, sp2), (ws, ws2)):
        assert first is None or torch.equal(first.view.view(torch.int32), second.view.view(torch.int32))
    del dq2, dw2, sp2, ws2
    # an empty workgroup's partials are zeros: of the weight gradient, of the sums, of LIN4's G
    live = d["g"] - d["empty"]
    if d["empty"]:
        assert not bool(ws.view.view(d["g"], m * k)[live:].any())
        if sums:
            assert not bool(sp.view.view(k, parts, 2)[:, 2 * live:].any())
        if qmode == C.OP_LIN4:
            assert not bool(dq.view.view(parts, 64, 4)[2 * live:].any())
    del ws

    # ---- once through the wrapper: the same bits
    kw, xkw = _operands(K, form, inp, fwd)
    w_dx, w_dw, below = K.gemm_backward_fused(inp["w"], xkw.pop("x"), need_dx=dgrad or qmode == C.OP_LIN4,
                                              **dict(kw, **xkw))
    assert torch.equal(w_dw.view(-1), dw.view)
    assert (below is not None) == sums
    if qmode == C.OP_LIN4:
        assert torch.equal(w_dx.partials.view(-1), dq.view)
    elif dgrad:
        assert torch.equal(w_dx.view(-1), dq.view)
    else:
        assert w_dx is None and dq is None

    # ---- numbers
    got = {"dw": dw.view.view(m, k)}
    if dgrad:
        got["dx"] = dq.view.view(b, k, r)
    if sums:
        part = sp.view.view(k, parts, 2).double()
        got.update(s_one=part[:, :, 0].sum(1), s_xhat=part[:, :, 1].sum(1))
        # mlp_bn_backward_finalize (the wrapper's): dgamma, dbeta, and coef as the (k,3) array the kernels read
        coef = below[2].contiguous().view(-1).view(k, 3)
        got.update(dgamma=below[0], dbeta=below[1], coef0=coef[:, 0], coef1=coef[:, 1], coef2=coef[:, 2])
    if qmode == C.OP_LIN4:
        got["G"] = dq.view.view(parts, 64, 4).double().sum(0)
        got["dw0"] = K.wgrad_first4_from_gated(inp["w0"], w_dx, fwd["meanx"], fwd["invx"], below[2],
                                               _moments(inp["x4"]))
    del w_dx, w_dw
    ref = C.reference64(form, inp, fwd)
    p32 = C.plain_fp32(form, inp, fwd)
    floors = C.resolution(form, inp, fwd, ref)
    if not dgrad:
        ref.pop("dx"), p32.pop("dx")
        if qmode != C.OP_LIN4:
            assert set(ref) == {"dw"}   # (128,259) without dq: the same dw truth as with it
    # what is compared with what, and which floor it gets
    names = {"dx": "dx", "dw": "dw", "s_one": "s_one", "s_xhat": "s_xhat", "dbeta": "s_one", "dgamma": "s_xhat",
             "G": "G", "dw0": "dw0"}
    pairs = [(n, ref[t], p32[t], floors.get(t, (0.0, 0.0))) for n, t in names.items() if n in got]
    if sums:
        for c, t in ((0, None), (1, "s_one"), (2, "s_xhat")):
            pairs.append(("coef%d" % c, ref["coef"][:, c], p32["coef"][:, c], floors.get(t, (0.0, 0.0))))
    if C.fused_shape(m, k)["xyz"] and dgrad:   # the three coordinate rows on their own (the vector ALU's)
        pairs.append(("xyz", ref["dx"][:, :3], p32["dx"][:, :3], (0.0, 0.0)))
        got["xyz"] = got["dx"][:, :3]
    bad = []
    for name, truth, yard, floor in pairs:
        e, e32 = C.errors(got[name], truth), C.errors(yard, truth)
        bound = C.bound_of(e32, (floor[0], floor[1] + C.ULP))
        # how much of the floor from `resolution` the figure needs (0: none; above 1 it fails)
        need = max([0.0] + [(e[i] - C.RATIO * e32[i] - (C.ULP if i else 0.0)) / floor[i] for i in (0, 1) if floor[i] > 0])
        print("bwd_fused %-7s (%d, %d, %d) T %d open %.3f %-6s kernel rel-L2 %.2e max/range %.2e | fp32 torch %.2e %.2e"
              " | floor %.2e %.2e need %.2f | bound %.2e %.2e" % ((form, b, groups, ns, d["T"], info["open"], name) + e + e32
                                                                   + tuple(floor) + (need,) + bound))
        if not (e[0] <= bound[0] and e[1] <= bound[1]):
            bad.append((name, e, e32, bound))
        if not e[1] <= CAPS[name]:
            bad.append((name, "cap", e))
    assert not bad, bad
