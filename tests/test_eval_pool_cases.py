"""tests/eval_pool_cases.py checks itself on the CPU: the float64 truth is the module it stands for, the
listed tile arithmetic is right, the shapes pass the gates, the tail / boundary cases are what their
names say, the planted groups exist and the fp32 yardstick is fp32-grade."""
import pytest
import torch

import eval_pool_cases as C


def _sequential(form, wts):
    """conv(1x1, no bias) / BatchNorm2d(eval) / ReLU in float64 whose folded affines are wts's: a
    random running mean and variance per channel, gamma and beta solved for (scale, shift)"""
    g = torch.Generator().manual_seed(5)
    mods = []
    for w, (scale, shift) in C._layers(form, wts):
        c = scale.numel()
        if w is not None:
            conv = torch.nn.Conv2d(w.shape[1], c, 1, bias=False).double()
            conv.weight.data.copy_(w.double().view(c, -1, 1, 1))
            mods.append(conv)
        bn = torch.nn.BatchNorm2d(c).double()
        var = 0.3 + 2 * torch.rand(c, generator=g, dtype=torch.float64)
        mean = torch.randn(c, generator=g, dtype=torch.float64)
        bn.running_var.copy_(var)
        bn.running_mean.copy_(mean)
        bn.weight.data.copy_(scale.double() * torch.sqrt(var + bn.eps))
        bn.bias.data.copy_(shift.double() + mean * scale.double())
        mods += [bn, torch.nn.ReLU()]
    return torch.nn.Sequential(*mods).eval()


@pytest.mark.parametrize("form,c_out,b,m,ns", [("lin4", 128, 2, 5, 16), ("stored", 256, 2, 3, 32)])
def test_truth_is_the_eval_module(form, c_out, b, m, ns):
    wts = C.weights(form, c_out, seed=1)
    x = (C.input_lin4 if form == "lin4" else C.input_stored)(b, m, ns, seed=1)
    out, pre = (C.truth_lin4 if form == "lin4" else C.truth_stored)(x, wts)
    with torch.no_grad():
        want = _sequential(form, wts)(x.double()).amax(3)
    assert out.dtype == torch.float64 and out.shape == (b, c_out, m)
    assert torch.allclose(out, want, rtol=1e-11, atol=1e-11 * want.abs().max().item())
    assert torch.equal(out, torch.relu(pre))


def test_listed_tile_arithmetic():
    for case, ns, b, m, tpw, tpc, total, wgs, live in C.STORED_SHAPES:
        if m is None:
            m = C.m_of_tiles(tpc, ns)
        assert tpw == (2 if ns == 64 or case == "c" else 1)
        assert C.tile_arith(b, m, ns, tpw) == (tpc, total, wgs, live), (case, ns)
        for c_out in (128, 256):
            assert C.stored_gate(b, c_out, m, ns)
    for case, ns, b, m, tpc, total, wgs in C.LIN4_SHAPES:
        assert C.tile_arith(b, m, ns, 2) == (tpc, total, wgs, 8), (case, ns)
        assert C.lin4_gate(b, m, ns)
    assert {(c, ns) for c, ns, *_ in C.STORED_SHAPES} == \
        {(c, ns) for c in "abd" for ns in (16, 32, 64)} | {("c", 16), ("c", 32)}


def test_tail_and_boundary_cases_are_what_they_say():
    seen_tail, seen_boundary = set(), set()
    for case, ns, b, m, tpw, tpc, total, wgs, live in C.STORED_SHAPES:
        if case in C.TAIL_CASES:
            assert total % (4 * tpw) != 0 and live < 4 * tpw, (case, ns)
            seen_tail.add(ns)
        if case in C.BOUNDARY_CASES:
            assert b > 1 and tpc % 4 != 0, (case, ns)
            seen_boundary.add(ns)
        if case == "c":
            assert tpc % 2 == 1  # a wave's pair of tiles straddles the boundary of clouds 0 and 1
    assert seen_tail == {16, 32, 64} and seen_boundary == {16, 32, 64}


def test_search_for_c_asks_only_the_query():
    calls = []

    def fake(b, c_out, m, ns):  # a chip whose rule is "two from 1000 tiles on"
        calls.append((b, c_out, m, ns))
        return 2 if b * m * ns // 32 >= 1000 else 1

    t = C.find_c_tiles(fake, 128, 16)
    assert t == 335 and (3 * t) % 8 != 0 and t % 2 == 1   # 3 * 333 = 999 < 1000; 3 * 335 = 1005, % 8 = 5
    assert all(c[0] == 3 and c[3] == 16 for c in calls)
    assert C.find_c_tiles(lambda b, c, m, ns: 2, 256, 32) == C.C_START_T


@pytest.mark.parametrize("form,c_out,ns", [("lin4", 128, 16), ("lin4", 128, 64), ("stored", 128, 16),
                                           ("stored", 256, 32), ("stored", 256, 64)])
def test_planted_groups_and_yardstick(form, c_out, ns):
    b, m = 3, 512 // ns
    wts = C.weights(form, c_out, seed=0)
    x = (C.input_lin4 if form == "lin4" else C.input_stored)(b, m, ns)
    out, pre = (C.truth_lin4 if form == "lin4" else C.truth_stored)(x, wts)
    neg = list(C.NEG_CH[c_out])
    assert (pre[:, neg] < -10).all() and (out[:, neg] == 0).all()   # every sample of every group
    assert (out > 0).float().mean() > 0.5                            # and the rest is alive
    for scale, _ in wts["coeff"]:
        frac = (scale < 0).float().mean().item()
        assert 0.08 < frac < 0.35, frac
    # the first affine cancels a mean of 40 in a few channels
    first = x[:, 3] if form == "lin4" else x[:, list(C.BIG_CH)]
    assert abs(first.mean().item() - C.BIG_MEAN) < 0.5
    assert C.rel_err(C.plain_fp32(form, x, wts), out) < 1e-5
