"""tests/bwd_fused_cases.py checks itself on the CPU: the mirror of the host logic gives the hand-computed
figures and is the library's (which loads without a device and then assumes 256 CUs), each form's table
reaches every edge of the persistent range split, the pooled form's lane arithmetic addresses every
column of a chunk at every admitted nsample, the seeded inputs meet their conditions, the dyadic LIN4
inputs recompute exactly, and reference64's closed forms are float64 autograd of the nn layer."""
import importlib

import pytest
import torch

from conftest import load_pkg
import bwd_fused_cases as C

FORM_NAMES = list(C.FORMS)
ROWS = [(f,) + c for f in FORM_NAMES for c in C.CASES[f]]

# per chunk count: (g, per, empty, lengths, last) at 256 CUs, worked out by hand; the cap of the two
# (64,64) forms is 512 (their row of the table has occ = 2), of the others 256
SPLITS = {
    64: (8, 8, 0, {8}, 8),
    65: (8, 9, 0, {9, 2}, 2),
    73: (9, 9, 0, {9, 1}, 1),
    75: (9, 9, 0, {9, 3}, 3),
    78: (9, 9, 0, {9, 6}, 6),
    89: (11, 9, 1, {9, 8}, 8),
    2057: (256, 9, 27, {9, 5}, 5),
    4112: (512, 9, 55, {9, 8}, 8),
}


def _K():
    load_pkg()
    return importlib.import_module("pointnet2._mlp_ext")


def test_the_seven_forms_are_the_dispatch():
    assert len(C.FORMS) == 7
    for name, (m, k, pmode, qmode, dgrad, sums) in C.FORMS.items():
        s = C.fused_shape(m, k)
        assert s is not None and (m, k) != (128, 128)
        assert sums == (k == 64) and (dgrad or (m, k) == (128, 259) or qmode == C.OP_LIN4)
        assert (qmode == C.OP_DIRECT) == (s["xyz"] == 3)
        for b, groups, ns, _ in C.CASES[name]:
            assert C.supported(b, m, k, groups * ns, pmode, qmode, ns if pmode == C.OP_POOLDY else 0) == 1
    assert len({v[:4] for v in C.FORMS.values()}) == 6   # (128,259) twice: with dq and without


def test_split_partitions_the_chunks():
    for cus in (1, 3, 104, 256, 304):
        for occ in (1, 2):
            for T in list(range(64, 700)) + [2056, 2057, 4112, 4625, 8192]:
                g = C.workgroups({"occ": occ}, T, cus)
                per, ranges = C.split(T, g)
                assert 1 <= g <= cus * occ and len(ranges) == g and T // g >= C.LEAST
                at = 0
                for lo, hi in ranges:
                    if lo < hi:
                        assert lo == at and hi - lo <= per
                        at = hi
                    else:
                        assert at == T
                assert at == T


def test_listed_figures():
    for form, b, groups, ns, _ in ROWS:
        d = C.describe(form, b, groups, ns)
        assert d["T"] in SPLITS, (form, b, groups, ns, d["T"])
        assert (d["g"], d["per"], d["empty"], d["lengths"], d["last"]) == SPLITS[d["T"]], (form, b, groups, ns)
        assert d["cap"] == (512 if form in ("bn64", "lin4") else 256)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_every_edge_of_a_form(form):
    rows = C.CASES[form]
    assert len(rows) == len({r[:3] for r in rows})
    ds = [C.describe(form, b, groups, ns) for b, groups, ns, _ in rows]
    assert any(d["T"] == 64 for d in ds)                                   # the smallest accepted size
    assert any(d["last"] == 1 and d["g"] > 1 for d in ds)                  # a last range of one chunk
    assert any(d["last"] == 2 and d["g"] > 1 for d in ds)                  # ... of two chunks
    assert any(n % 2 for d in ds for n in d["lengths"] if n >= 3)          # odd ranges
    assert any(n % 2 == 0 for d in ds for n in d["lengths"] if n >= 4)     # even ranges
    assert any(d["empty"] and d["g"] < d["cap"] for d in ds)               # an empty workgroup below the cap
    assert any(d["inside"] for d in ds)                                    # a cloud boundary inside a range
    assert any(b == 1 for b, _, _, _ in rows)
    cap = [d for d in ds if d["g"] == d["cap"]]                            # at the CU cap
    assert cap and all(d["per"] > 8 and d["empty"] > 0 and d["T"] // C.LEAST > d["cap"] for d in cap)
    m, k = C.FORMS[form][:2]
    for (b, groups, ns, _), d in zip(rows, ds):
        assert b * max(m, k) * groups * ns * 4 <= 70e6                     # the largest activation, bytes
    if form in C.POOL_NS:
        tn = C.fused_shape(m, k)["tn"]
        assert {ns for _, _, ns, _ in rows} == set(C.POOL_NS[form])
        assert any(ns > tn for _, _, ns, _ in rows) and any(ns < tn for _, _, ns, _ in rows)
        # a group that spans chunks also in a row with ragged ranges and cloud boundaries inside them
        assert any(ns > tn and d["inside"] and len(d["lengths"]) > 1 for (_, _, ns, _), d in zip(rows, ds))


@pytest.mark.parametrize("form", sorted(C.POOL_NS))
def test_pool_lane_addresses_every_column(form):
    m, k = C.FORMS[form][:2]
    tn = C.fused_shape(m, k)["tn"]
    for ns in range(16, 257, 16):
        r = 3 * ns * tn   # whole chunks and whole groups
        ok = bool(C.supported(2, m, k, r, C.OP_POOLDY, C.OP_BNRELU, ns))
        assert ok == (ns % tn == 0 or tn % ns == 0) and (ok or ns not in C.POOL_NS[form])
        if not ok:
            continue
        for col0 in range(0, r, tn):
            for seg_c in range(0, tn, 16):
                group, first = C.pool_lane(ns, tn, col0, seg_c)
                assert group * ns + first == col0 + seg_c and 0 <= first and first + 16 <= ns, (ns, col0, seg_c)


def test_mirror_is_the_library():
    """mlp_gemm_backward_fused_supported over a grid with the unsupported neighbours, and the two sizes
    for every row of every table (no device: fused_cus() falls back to 256)"""
    lib = _K()._lib
    seen = set()
    shapes = [row[:2] for row in C.TABLE] + [(96, 64), (64, 128), (128, 130)]
    for m, k in shapes:
        for b in (1, 2, 3):
            for r in (32, 63 * 32, 63 * 64, 2016, 2048, 2080, 4096, 4128, 64 * 96, 6144 + 16, 8192):
                for pmode in (0, 1, 2, 3, 4):
                    for qmode in (0, 1, 2, 4):
                        for ns in (0, 8, 16, 32, 48, 64, 96, 128, 256):
                            want = C.supported(b, m, k, r, pmode, qmode, ns)
                            assert int(lib.mlp_gemm_backward_fused_supported(b, m, k, r, pmode, qmode, ns)) == want, \
                                (b, m, k, r, pmode, qmode, ns)
                            seen.add(((m, k, pmode, qmode), want))
                assert int(lib.mlp_gemm_backward_fused_stats_parts(b, m, k, r)) == C.stats_parts(b, m, k, r)
                assert int(lib.mlp_gemm_backward_fused_workspace_floats(b, m, k, r)) == C.workspace_floats(b, m, k, r)
    for m, k, pmode, qmode, _, _ in C.FORMS.values():
        assert ((m, k, pmode, qmode), 1) in seen and ((m, k, pmode, qmode), 0) in seen
    # the named refusals: ns = 48, r no multiple of the chunk, T = 63, the wrong operand pairing
    for args in ((2, 128, 64, 48 * 64, 3, 1, 48), (2, 64, 64, 4096 + 32, 2, 1, 0), (1, 64, 64, 63 * 64, 2, 1, 0),
                 (1, 128, 131, 63 * 32, 2, 0, 0), (2, 128, 64, 4096, 2, 1, 0), (2, 64, 64, 4096, 3, 1, 64),
                 (2, 128, 131, 4096, 2, 1, 0), (2, 64, 64, 4096, 2, 0, 0), (2, 128, 64, 4096, 3, 4, 64),
                 (2, 256, 128, 48 * 64, 3, 1, 48)):
        assert C.supported(*args) == 0 and int(lib.mlp_gemm_backward_fused_supported(*args)) == 0, args
    for form, b, groups, ns, _ in ROWS:
        m, k, pmode, qmode, _, sums = C.FORMS[form]
        r = groups * ns
        d = C.describe(form, b, groups, ns)
        assert int(lib.mlp_gemm_backward_fused_supported(b, m, k, r, pmode, qmode, ns if pmode == 3 else 0)) == 1
        assert int(lib.mlp_gemm_backward_fused_stats_parts(b, m, k, r)) == C.stats_parts(b, m, k, r) == (2 * d["g"] if sums else 0)
        assert int(lib.mlp_gemm_backward_fused_workspace_floats(b, m, k, r)) == C.workspace_floats(b, m, k, r) == d["g"] * m * k


SMALL = [(f, b, groups, ns, seed) for f, b, groups, ns, seed in ROWS if C.chunks(f, b, groups, ns) <= 89]


@pytest.mark.parametrize("form,b,groups,ns,seed", SMALL)
def test_seeded_inputs_meet_their_conditions(form, b, groups, ns, seed):
    inp = C.make_inputs(form, b, groups, ns, seed)
    info = C.check_inputs(form, inp, C.forward64(form, inp))
    assert C.MIN_SHARE < info["open"] < 1 - C.MIN_SHARE
    if form == "lin4":   # the dyadic inputs recompute exactly, in fp32 arithmetic as well
        x4, w0 = inp["x4"].view(b, 4, -1), inp["w0"]
        acc = w0[:, 0].view(1, -1, 1) * x4[:, 0].unsqueeze(1)
        for c in (1, 2, 3):
            acc = acc + w0[:, c].view(1, -1, 1) * x4[:, c].unsqueeze(1)   # (every product exact: no fused op needed)
        assert torch.equal(acc, inp["x"].view(b, 64, -1)) and info["lin4_margin"] > C.LIN4_MARGIN


def _module_grads(form, inp, fwd):
    """Conv2d 1x1 (no bias) / BatchNorm2d (training) / ReLU (/ max over nsample, gathered at the given
    winners) in float64 with autograd, on the layer's input as a leaf -> (dx, dw, dw0 or None)"""
    m, k, pmode, qmode, _, _ = C.FORMS[form]
    b, groups, ns = inp["b"], inp["groups"], inp["ns"]
    conv = torch.nn.Conv2d(k, m, 1, bias=False).double()
    conv.weight.data.copy_(inp["w"].double().view(m, k, 1, 1))
    bn = torch.nn.BatchNorm2d(m, eps=C.EPS).double().train()
    bn.weight.data.copy_(inp["g"].double())
    bn.bias.data.copy_(inp["be"].double())
    x = inp["x"].double()
    w0 = None
    if qmode == C.OP_LIN4:
        conv0 = torch.nn.Conv2d(4, 64, 1, bias=False).double()
        conv0.weight.data.copy_(inp["w0"].double().view(64, 4, 1, 1))
        w0 = conv0.weight
        x = conv0(inp["x4"].double())
    if qmode != C.OP_DIRECT:
        bnx = torch.nn.BatchNorm2d(k, eps=C.EPS).double().train()
        bnx.weight.data.copy_(inp["gx"].double())
        bnx.bias.data.copy_(inp["bex"].double())
        a = torch.relu(bnx(x))
    else:
        a = x.clone().requires_grad_(True)
    a.retain_grad()
    act = torch.relu(bn(conv(a)))
    if pmode == C.OP_POOLDY:
        act = torch.gather(act, 3, fwd["argmax"].long().unsqueeze(-1)).squeeze(-1)
    (act * inp["dz"].double()).sum().backward()
    return (a.grad.view(b, k, groups * ns), conv.weight.grad.view(m, k),
            w0.grad.view(64, 4) if w0 is not None else None)


@pytest.mark.parametrize("form,b,groups,ns", [("bn64", 2, 5, 64), ("lin4", 2, 3, 64), ("pool64", 2, 7, 16),
                                              ("pool64", 1, 3, 128), ("pool128", 2, 5, 96), ("pool128", 2, 9, 16),
                                              ("xyz131", 2, 3, 32), ("xyz259", 1, 3, 32)])
def test_closed_forms_are_the_modules_autograd(form, b, groups, ns):
    """On float64 statistics (forward64 with rounded=False) reference64 is autograd of the nn layer to the
    last bits; on the fp32-rounded ones it is the same up to those roundings, and plain fp32 is fp32-grade"""
    inp = C.make_inputs(form, b, groups, ns, 0)
    exact = C.forward64(form, inp, rounded=False)
    ref = C.reference64(form, inp, exact)
    dx, dw, dw0 = _module_grads(form, inp, exact)
    for name, want in (("dx", dx), ("dw", dw)) + ((("dw0", dw0),) if dw0 is not None else ()):
        assert float((ref[name] - want).abs().max()) <= 1e-11 * float(want.abs().max()), name
    if "s_one" in ref:   # the layer below's dbeta, dgamma: what its BatchNorm module would get
        bnx = _module_below(form, inp)
        assert float((ref["s_one"] - bnx[1]).abs().max()) <= 1e-11 * float(bnx[1].abs().max())
        assert float((ref["s_xhat"] - bnx[0]).abs().max()) <= 1e-11 * float(bnx[0].abs().max())
    fwd = C.forward64(form, inp)
    C.check_inputs(form, inp, fwd, coverage=False)
    rounded = C.reference64(form, inp, fwd)
    p32 = C.plain_fp32(form, inp, fwd)
    assert set(p32) == set(rounded)
    for name in rounded:
        assert max(C.errors(rounded[name], ref[name])) < 5e-6, (name, C.errors(rounded[name], ref[name]))
        assert max(C.errors(p32[name], rounded[name])) < 2e-5, (name, C.errors(p32[name], rounded[name]))


def _module_below(form, inp):
    """(weight.grad, bias.grad) of the layer below's BatchNorm2d in the whole two-layer module"""
    m, k, pmode, qmode, _, _ = C.FORMS[form]
    x = inp["x"].double()
    bnx = torch.nn.BatchNorm2d(k, eps=C.EPS).double().train()
    bnx.weight.data.copy_(inp["gx"].double())
    bnx.bias.data.copy_(inp["bex"].double())
    bn = torch.nn.BatchNorm2d(m, eps=C.EPS).double().train()
    bn.weight.data.copy_(inp["g"].double())
    bn.bias.data.copy_(inp["be"].double())
    act = torch.relu(bn(torch.nn.functional.conv2d(torch.relu(bnx(x)), inp["w"].double().view(m, k, 1, 1))))
    if pmode == C.OP_POOLDY:
        exact = C.forward64(form, inp, rounded=False)
        act = torch.gather(act, 3, exact["argmax"].long().unsqueeze(-1)).squeeze(-1)
    (act * inp["dz"].double()).sum().backward()
    return bnx.weight.grad, bnx.bias.grad
