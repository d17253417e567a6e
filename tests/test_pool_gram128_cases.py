"""tests/pool_gram128_cases.py checks itself on the CPU: the mirror of the range split gives the hand-
computed figures, the table reaches every edge of the persistent pass for each nsample and every form
of the reduce loop at 256 CUs, the seeded inputs meet their conditions, the float64 truth is the
reference's module, the pass's own formulas agree with it, and the rule of the GPU test (three times
plain fp32's own error plus the format's floors) passes the kernel's arithmetic -- three bf16 terms, six
of the nine partial products -- and fails it with a term or a product less."""
import pytest
import torch

import pool_gram128_cases as C

ROWS = [c[:3] for c in C.CASES]

# (b, m, ns): T, workgroups, per, empty ranges, lengths of the others, crossing ranges, groups split
# between workgroups, (four-wide, single) iterations of the reduce slices; worked out by hand for 256 CUs
LISTED = {
    (1, 128, 16): (64, 8, 8, 0, {8}, 0, 0, {(0, 1)}),
    (1, 64, 32): (64, 8, 8, 0, {8}, 0, 0, {(0, 1)}),
    (1, 32, 64): (64, 8, 8, 0, {8}, 0, 0, {(0, 1)}),
    (1, 146, 16): (73, 9, 9, 0, {9, 1}, 0, 0, {(0, 1), (0, 2)}),
    (1, 73, 32): (73, 9, 9, 0, {9, 1}, 0, 0, {(0, 1), (0, 2)}),
    (1, 41, 64): (82, 10, 9, 0, {9, 1}, 0, 5, {(0, 1), (0, 2)}),
    (3, 54, 16): (81, 10, 9, 1, {9}, 0, 0, {(0, 1), (0, 2)}),
    (3, 27, 32): (81, 10, 9, 1, {9}, 0, 0, {(0, 1), (0, 2)}),
    (5, 13, 32): (65, 8, 9, 0, {9, 2}, 4, 0, {(0, 1)}),
    (3, 11, 64): (66, 8, 9, 0, {9, 3}, 2, 4, {(0, 1)}),
    (3, 67, 32): (201, 25, 9, 2, {9, 3}, 2, 0, {(1, 0), (0, 3)}),
    (5, 21, 64): (210, 26, 9, 2, {9, 3}, 3, 12, {(1, 0), (0, 3)}),
    (3, 88, 32): (264, 33, 8, 0, {8}, 0, 0, {(1, 0), (1, 1)}),
    (2, 514, 64): (2056, 256, 9, 27, {9, 4}, 1, 114, {(8, 0)}),
    (2, 2056, 16): (2056, 256, 9, 27, {9, 4}, 1, 0, {(8, 0)}),
    (2, 2056, 32): (4112, 256, 17, 14, {17, 15}, 1, 0, {(8, 0)}),
}
FIGURES = ("T", "g", "per", "empty", "lengths", "crossing", "group_split", "reduce_form")


def test_split_partitions_the_chunks():
    for cus in (1, 3, 104, 256, 304):
        for T in list(range(64, 701)) + [2056, 4112]:
            g, per, ranges = C.split(T, C.LEAST, cus)
            assert 1 <= g <= cus and len(ranges) == g and (g == 1 or T // g >= C.LEAST)
            at = 0
            for lo, hi in ranges:   # in order, without gaps; what is left over is empty ranges at the end
                if lo < hi:
                    assert lo == at and hi - lo <= per
                    at = hi
                else:
                    assert at == T
            assert at == T


def test_listed_figures():
    assert set(ROWS) == set(LISTED) and len(ROWS) == len(set(ROWS))
    for row in ROWS:
        d = C.describe(*row)
        assert C.chunks(*row) == d["T"]
        assert tuple(d[name] for name in FIGURES) == LISTED[row], row
    assert C.reduce_form(1) == {(0, 1), (0, 0)} and C.reduce_form(24) == {(0, 3)} and C.reduce_form(57) == {(2, 0), (1, 3)}


def test_rows_are_covered_and_small():
    for b, m, ns in ROWS:
        assert C.covers(b, m * ns, ns)
        assert b * C.K_IN * m * ns * 4 <= 35e6   # y2, bytes
        # the float64 reference's largest tensors: y3 and its kin (b, 128, r); a handful are alive at once
        assert b * C.M_OUT * m * ns * 8 * 3 < 0.5e9
        assert C.workspace_floats(b, m, ns) % 2 == 0
    assert set(C.SPARSE_ONLY) <= set(ROWS) and sorted(ns for _, _, ns in C.SPARSE_ONLY) == [16, 32, 64]
    for b, m, ns in C.SPARSE_ONLY:   # (gram_form64 holds S dense)
        assert C.chunks(b, m, ns) <= 100


@pytest.mark.parametrize("ns", [16, 32, 64])
def test_every_edge_of_the_pass(ns):
    ds = [C.describe(b, m, n) for b, m, n in ROWS if n == ns]
    assert any(d["empty"] for d in ds)
    # a range of one chunk behind full ranges: T = (g - 1) per + 1
    assert any(1 in d["lengths"] and d["T"] == (d["g"] - 1) * d["per"] + 1 for d in ds)
    assert any(n >= 3 and n % 2 for d in ds for n in d["lengths"])
    assert any(n % 2 == 0 for d in ds for n in d["lengths"])
    assert any(d["crossing"] for d in ds)
    assert any(d["g"] < C.CUS for d in ds)
    assert any(d["T"] // C.LEAST > C.CUS and d["g"] == C.CUS for d in ds)
    assert any(d["T"] == C.MIN_CHUNKS for d in ds)   # the smallest covered shape
    if ns == 64:
        assert any(d["group_split"] for d in ds)
        # a range that ends inside a group AND one that ends between groups
        assert any(0 < d["group_split"] < d["g"] - d["empty"] - 1 for d in ds)
    else:
        assert not any(d["group_split"] for d in ds)


def test_every_reduce_form():
    forms = set().union(*(C.describe(*row)["reduce_form"] for row in ROWS))
    assert any(wide == 0 and single > 0 for wide, single in forms)    # no four-wide iteration
    assert any(wide > 0 and single > 0 for wide, single in forms)     # mixed
    assert any(wide > 0 and single == 0 for wide, single in forms)    # only four-wide iterations
    assert any(wide > 1 for wide, _ in forms) and any(single > 1 for _, single in forms)   # each loop goes round


def test_refusal_shapes():
    assert C.covers(1, 64 * 32, 32)
    assert not C.covers(1, 63 * 32, 32)          # T = 63
    assert not C.covers(1, 256 * 8, 8)           # ns = 8
    assert not C.covers(1, 16 * 128, 128)        # ns = 128
    assert not C.covers(1, 129 * 16, 16)         # r % 32 != 0
    assert not C.covers(1, 2080, 64)             # r % ns != 0
    assert 2080 % 32 == 0 and 2080 // 32 >= C.MIN_CHUNKS and 129 * 16 // 32 >= C.MIN_CHUNKS


@pytest.mark.parametrize("b,m,ns,seed", C.CASES)
def test_seeded_inputs_meet_their_conditions(b, m, ns, seed):
    assert b * C.M_OUT * m * ns * 8 * 3 < 0.5e9   # (the size guard: float64 tensors of y3's extent on the CPU)
    inp = C.make_inputs(b, m, ns, seed)
    info = C.check_inputs(inp, C.forward64(inp))
    assert info["shut"] > C.MIN_SHARE and min(info["meet"].values()) > 0
    # every fifth BatchNorm weight negative on both layers, every seventh layer-3 channel biased shut
    assert bool((inp["g2"][::5] < 0).all()) and bool((inp["g3"][::5] < 0).all())
    assert int((inp["g2"] < 0).sum()) == 13 and int((inp["g3"] < 0).sum()) == 26
    assert float(inp["be3"][2::7].mean()) < -1.5 < -0.5 < float(inp["be3"].mean())
    # twin columns in every third group
    assert torch.equal(inp["y2"][:, :, ::C.TWIN_EVERY, 3], inp["y2"][:, :, ::C.TWIN_EVERY, 1])
    assert not torch.equal(inp["y2"][:, :, 1::C.TWIN_EVERY, 3], inp["y2"][:, :, 1::C.TWIN_EVERY, 1])


def _module_grads(inp, fwd):
    """Conv2d 1x1 (no bias) / BatchNorm2d (training) / ReLU / max over nsample in float64, on a2 as a leaf"""
    b, m, ns = inp["b"], inp["m"], inp["ns"]
    conv = torch.nn.Conv2d(C.K_IN, C.M_OUT, 1, bias=False).double()
    conv.weight.data.copy_(inp["w3"].double().view(C.M_OUT, C.K_IN, 1, 1))
    bn = torch.nn.BatchNorm2d(C.M_OUT, eps=C.EPS).double().train()
    bn.weight.data.copy_(inp["g3"].double())
    bn.bias.data.copy_(inp["be3"].double())
    a2 = torch.relu(inp["y2"].double() * fwd["sc2"].double().view(1, -1, 1, 1) + fwd["sh2"].double().view(1, -1, 1, 1))
    a2.requires_grad_(True)
    pooled = torch.nn.functional.max_pool2d(torch.relu(bn(conv(a2))), kernel_size=[1, ns]).squeeze(-1)
    (pooled * inp["dpooled"].double()).sum().backward()
    return a2.grad.view(b, C.K_IN, m * ns), conv.weight.grad.view(C.M_OUT, C.K_IN)


@pytest.mark.parametrize("b,m,ns,seed", [c for c in C.CASES if c[:3] in C.SPARSE_ONLY])
def test_truth_is_the_module_and_the_formulas_agree(b, m, ns, seed):
    inp = C.make_inputs(b, m, ns, seed)
    fwd = C.forward64(inp)
    ref = C.reference64(inp, fwd)
    dq, dw = _module_grads(inp, fwd)
    # the twin columns (1 and 3 of every third group) hold one number twice: which of them the module's
    # pool credits is its own choice, and the weight gradient does not depend on it
    keep = torch.ones(b, C.K_IN, m, ns, dtype=torch.bool)
    keep[:, :, ::C.TWIN_EVERY, 1] = False
    keep[:, :, ::C.TWIN_EVERY, 3] = False
    keep = keep.view(b, C.K_IN, m * ns)
    assert torch.allclose(ref["dq"][keep], dq[keep], rtol=0, atol=1e-11 * dq.abs().max().item())
    pair = lambda t: t.view(b, C.K_IN, m, ns)[:, :, ::C.TWIN_EVERY, [1, 3]].sum(-1)  # noqa: E731
    assert torch.allclose(pair(ref["dq"]), pair(dq), rtol=0, atol=1e-11 * dq.abs().max().item())
    assert torch.allclose(ref["dw"], dw, rtol=0, atol=1e-11 * dw.abs().max().item())
    # the pass's formulas with every term and every product: the truth up to the fp32 roundings of the
    # statistics, of q, p, M3, v and of a dpooled
    own = C.gram_form64(inp, fwd, terms=3, products=[(i, j) for i in range(3) for j in range(3)])
    for name in ("dq", "dw"):
        e = C.errors(torch.from_numpy(own[name]), ref[name])
        assert max(e) < 2e-6, (name, e)   # (pool_gram256_cases' figure for the same roundings)
    # and plain fp32 is fp32-grade
    p32 = C.plain_fp32(inp, fwd)
    for name in C.OUTPUTS:
        assert max(C.errors(p32[name], ref[name])) < 2e-5, name
    # sparse only: the truth is W3^T S and S a2^T, and the formulas give them to float64 rounding apart
    # from the one fp32 rounding of a dpooled
    fwd0 = C.forward64(inp, sparse_only=True)
    assert bool((fwd0["coef3"][:, 1:] == 0).all()) and torch.equal(fwd0["coef3"][:, 0], fwd["coef3"][:, 0])
    assert torch.equal(fwd0["argmax"], fwd["argmax"])
    ref0 = C.reference64(inp, fwd0)
    open_ = (fwd["ymax"].double() * fwd["sc3"].double().view(1, -1, 1) + fwd["sh3"].double().view(1, -1, 1)) > 0
    s = torch.zeros(b, C.M_OUT, m, ns, dtype=torch.float64)
    s.scatter_(3, fwd["argmax"].long().unsqueeze(-1), torch.where(
        open_, (inp["g3"].double() / torch.sqrt(_var3(inp, fwd) + C.EPS)).view(1, -1, 1) * inp["dpooled"].double(),
        torch.zeros((), dtype=torch.float64)).unsqueeze(-1))
    s = s.view(b, C.M_OUT, m * ns)
    a2 = torch.relu(inp["y2"].double().view(b, C.K_IN, -1) * fwd["sc2"].double().view(1, -1, 1) + fwd["sh2"].double().view(1, -1, 1))
    assert max(C.errors(torch.einsum("ok,bor->bkr", inp["w3"].double(), s), ref0["dq"])) < 1e-13
    assert max(C.errors(torch.einsum("bor,bkr->ok", s, a2), ref0["dw"])) < 1e-13
    own0 = C.gram_form64(inp, fwd0, terms=3, products=[(i, j) for i in range(3) for j in range(3)])
    for name in ("dq", "dw"):
        assert max(C.errors(torch.from_numpy(own0[name]), ref0[name])) < 2e-7, name


def _var3(inp, fwd):
    b, r = inp["b"], inp["r"]
    a2 = torch.relu(inp["y2"].double().view(b, C.K_IN, r) * fwd["sc2"].double().view(1, -1, 1) + fwd["sh2"].double().view(1, -1, 1))
    return torch.einsum("ok,bkr->bor", inp["w3"].double(), a2).var(dim=(0, 2), unbiased=False)


# ------------------------------------------------------------------ the bound discriminates
@pytest.fixture(scope="module")
def small_row():
    """T = 73, ns = 32: inputs, both forwards, truths and yardsticks, computed once and left unchanged"""
    b, m, ns, seed = [c for c in C.CASES if c[:3] == (1, 73, 32)][0]
    inp = C.make_inputs(b, m, ns, seed)
    out = {"inp": inp}
    for mode in (False, True):
        fwd = C.forward64(inp, sparse_only=mode)
        ref = C.reference64(inp, fwd)
        p32 = C.plain_fp32(inp, fwd)
        out[mode] = (fwd, ref, {name: C.errors(p32[name], ref[name]) for name in ("dq", "dw")})
    return out


def _judge(small_row, mode, label, **form):
    """-> {output: passes the GPU test's rule}, the figures printed"""
    fwd, ref, e32 = small_row[mode]
    got = C.gram_form64(small_row["inp"], fwd, **form)
    verdict = {}
    for name in ("dq", "dw"):
        e = C.errors(torch.from_numpy(got[name]), ref[name])
        verdict[name], bound = C.within(name, e, e32[name])
        print("%-28s %s rel-L2 %.2e max/range %.2e | fp32 torch %.2e %.2e | bound %.2e %.2e -> %s" % (
            (label, name) + e + e32[name] + bound + ("passes" if verdict[name] else "FAILS",)))
    return verdict


@pytest.mark.parametrize("mode", [False, True], ids=["dense", "sparse_only"])
def test_bound_passes_the_kernels_arithmetic(small_row, mode):
    """three bf16 terms, the six kept products, everything else in float64"""
    assert all(_judge(small_row, mode, "3 terms, 6 products", terms=3, products=C.SIX).values())


@pytest.mark.parametrize("mode", [False, True], ids=["dense", "sparse_only"])
def test_bound_fails_a_two_term_split(small_row, mode):
    """the operands cut to two bf16 terms (16 mantissa bits): both outputs miss the bound"""
    verdict = _judge(small_row, mode, "2 terms", terms=2, products=C.SIX)
    assert not verdict["dq"] and not verdict["dw"], verdict


@pytest.mark.parametrize("dropped", [p for p in C.SIX if p != (C.HI, C.HI)], ids=lambda p: "no_%d%d" % p)
def test_bound_fails_five_of_the_six_products(small_row, dropped):
    """any one of the five small partial products left out (2^-16 to 2^-8 of the product): both outputs
    miss the bound"""
    five = [p for p in C.SIX if p != dropped]
    verdict = _judge(small_row, False, "without product (%d, %d)" % dropped, terms=3, products=five)
    assert not verdict["dq"] and not verdict["dw"], verdict


def test_bound_fails_a_two_term_sparse_image(small_row):
    """sparse_only: S alone cut to two terms (the third term of a dpooled never reaches its image) -- the
    dense part is zero and cannot mask it: both outputs miss the bound"""
    verdict = _judge(small_row, True, "sparse_only, S in 2 terms", terms=3, products=C.SIX, s_terms=2)
    assert not verdict["dq"] and not verdict["dw"], verdict
