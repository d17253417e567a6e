"""tests/pool_gram256_cases.py checks itself on the CPU: the mirror of the range split gives the hand-
computed figures, the table reaches every edge of both persistent passes and of the reduce loop at 256
CUs, the seeded inputs meet their conditions, the float64 truth is the reference's module, the pass's
own formulas agree with it, and the bound of the GPU test (three times plain fp32's own error) is
tight enough to fail a kernel that drops the third bf16 term of its operands."""
import numpy as np
import pytest
import torch

import pool_gram256_cases as C

ROWS = [c[:3] for c in C.CASES]
PASSES = (("data", C.DGRAD_LEAST), ("weight", C.WGRAD_LEAST))

# (b, m, ns): T, then per pass (workgroups, per, empty ranges, lengths of the others, crossing ranges),
# worked out by hand for 256 CUs
LISTED = {
    (1, 1, 32): (1, (1, 1, 0, {1}, 0), (1, 1, 0, {1}, 0)),
    (1, 2, 16): (1, (1, 1, 0, {1}, 0), (1, 1, 0, {1}, 0)),
    (1, 3, 32): (3, (1, 3, 0, {3}, 0), (1, 3, 0, {3}, 0)),
    (2, 64, 16): (64, (8, 8, 0, {8}, 0), (4, 16, 0, {16}, 0)),
    (3, 27, 32): (81, (10, 9, 1, {9}, 0), (5, 17, 0, {13, 17}, 2)),
    (17, 17, 32): (289, (36, 9, 3, {1, 9}, 15), (18, 17, 1, {17}, 0)),
    (3, 50, 16): (75, (9, 9, 0, {3, 9}, 2), (4, 19, 0, {18, 19}, 2)),
    (2, 330, 16): (330, (41, 9, 4, {6, 9}, 1), (20, 17, 0, {7, 17}, 1)),
    (2, 201, 32): (402, (50, 9, 5, {6, 9}, 1), (25, 17, 1, {11, 17}, 1)),
    (5, 129, 32): (645, (80, 9, 8, {6, 9}, 3), (40, 17, 2, {16, 17}, 4)),
    (2, 460, 16): (460, (57, 9, 5, {1, 9}, 1), (28, 17, 0, {1, 17}, 1)),
    (5, 92, 32): (460, (57, 9, 5, {1, 9}, 4), (28, 17, 0, {1, 17}, 4)),
    (1, 4112, 16): (2056, (256, 9, 27, {4, 9}, 0), (128, 17, 7, {16, 17}, 0)),
    (2, 2056, 32): (4112, (256, 17, 14, {15, 17}, 1), (256, 17, 14, {15, 17}, 1)),
}


def test_split_partitions_the_chunks():
    for cus in (1, 3, 104, 256, 304):
        for least in (C.DGRAD_LEAST, C.WGRAD_LEAST):
            for T in list(range(1, 700)) + [2056, 4112, 8192, 16384]:
                g, per, ranges = C.split(T, least, cus)
                assert 1 <= g <= cus and len(ranges) == g and (g == 1 or T // g >= least)
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
        T, *listed = LISTED[row]
        assert C.chunks(*row) == T
        for (_, least), want in zip(PASSES, listed):
            d = C.describe(*row, least)
            assert (d["g"], d["per"], d["empty"], d["lengths"], d["crossing"]) == want, (row, least)


def test_rows_are_covered_and_small():
    for b, m, ns in ROWS:
        assert C.covers(b, m * ns, ns)
        assert b * C.K_IN * m * ns * 4 <= 70e6   # y2, bytes
        # the float64 reference's largest tensors: y3 and its kin (b, 256, r); a handful are alive at once
        assert b * C.M_OUT * m * ns * 8 * 3 < 1e9
        assert C.workspace_floats(b, m, ns) % 2 == 0   # the sums' doubles sit 8-byte aligned in the workspace
        assert C.records_offset_floats() % 4 == 0 and C.sums_offset_floats(b, m, ns) % 2 == 0


@pytest.mark.parametrize("ns", [16, 32])
@pytest.mark.parametrize("name,least", PASSES)
def test_every_edge_of_a_pass(name, least, ns):
    ds = [C.describe(b, m, n, least) for b, m, n in ROWS if n == ns]
    assert any(d["empty"] for d in ds)
    assert any(1 in d["lengths"] for d in ds)
    # a range of one chunk behind others: it begins inside the tensor, behind a full range
    assert any(1 in d["lengths"] and d["g"] > 1 for d in ds)
    assert any(n >= 3 and n % 2 for d in ds for n in d["lengths"])
    assert any(n % 2 == 0 for d in ds for n in d["lengths"])
    assert any(d["crossing"] for d in ds)


def test_grid_cap_reduce_forms_and_pack_blocks():
    for _, least in PASSES:
        assert any(C.chunks(*row) // least > C.CUS and C.describe(*row, least)["g"] == C.CUS for row in ROWS)
        assert any(C.describe(*row, least)["g"] < C.CUS for row in ROWS)
    parts = {C.describe(*row, C.WGRAD_LEAST)["g"] for row in ROWS}
    assert 1 in parts and 25 in parts and 256 in parts   # 25: only slice 0 enters the four-at-a-time loop
    assert any(2 <= p <= 8 for p in parts) and any(9 <= p <= 24 for p in parts)
    assert any(33 <= p <= 255 for p in parts)
    assert any(m % 32 for _, m, _ in ROWS) and any(m % 32 == 0 for _, m, _ in ROWS)
    # two groups per chunk and one
    assert {ns for _, _, ns in ROWS} == {16, 32}


@pytest.mark.parametrize("b,m,ns,seed", C.CASES)
def test_seeded_inputs_meet_their_conditions(b, m, ns, seed):
    inp = C.make_inputs(b, m, ns, seed)
    info = C.check_inputs(inp, C.forward64(inp))
    assert info["shut"] > C.MIN_SHARE
    # every fifth BatchNorm weight negative, on both layers
    assert bool((inp["g2"][::5] < 0).all()) and bool((inp["g3"][::5] < 0).all())
    assert int((inp["g2"] < 0).sum()) == 26 and int((inp["g3"] < 0).sum()) == 52


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


@pytest.mark.parametrize("b,m,ns,seed", [(3, 27, 32, 0), (3, 50, 16, 0), (1, 2, 16, 0)])
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
    # the pass's formulas on the fp32-rounded statistics: the truth up to those roundings
    own = C.gram_form64(inp, fwd, terms=3)
    for name in ("dq", "dw"):
        e = C.errors(torch.from_numpy(own[name]), ref[name])
        assert max(e) < 2e-6, (name, e)
    # and plain fp32 is fp32-grade
    p32 = C.plain_fp32(inp, fwd)
    for name in C.OUTPUTS:
        assert max(C.errors(p32[name], ref[name])) < 2e-5, name


def test_bound_fails_a_two_term_split():
    """At T = 81: the products the kernels form from the bf16 images of a2, with a2 cut to two terms (16
    mantissa bits), miss the exact products by more than three times what fp32 numpy misses them by --
    and the weight gradient built from them misses the bound of the GPU test."""
    b, m, ns, seed = [c for c in C.CASES if C.chunks(*c[:3]) == 81][0]
    assert C.chunks(b, m, ns) == 81
    inp = C.make_inputs(b, m, ns, seed)
    fwd = C.forward64(inp)
    two = C.gram_form64(inp, fwd, terms=2)

    def err(got, truth):
        d = got.astype(np.float64) - truth
        return np.linalg.norm(d) / np.linalg.norm(truth), np.abs(d).max() / np.abs(truth).max()

    for name in ("m3a2", "gram"):
        e2, e32 = err(two[name], two[name + "_exact"]), err(two[name + "_fp32"], two[name + "_exact"])
        print("two-term %s: rel-L2 %.2e max/range %.2e; fp32 numpy %.2e %.2e" % ((name,) + e2 + e32))
        assert e2[0] > C.RATIO * e32[0] and e2[1] > C.RATIO * e32[1], (name, e2, e32)
    # The pass's outputs under the GPU test's bound.  dw takes the cut operand whole (the Gram matrix and
    # S a2^T) and misses the bound twenty times over.  dq does not: its dense term M3 a2 is a small part
    # of it next to W3^T S, whose operands are not a2's images, so the cut moves dq by about what plain
    # fp32 itself is off by (printed, not asserted; DESIGN.md says so)
    ref = C.reference64(inp, fwd)
    p32 = C.plain_fp32(inp, fwd)
    for name in ("dq", "dw"):
        e2 = C.errors(torch.from_numpy(two[name]), ref[name])
        bound = C.bound_of(C.errors(p32[name], ref[name]))
        print("two-term %s: rel-L2 %.2e max/range %.2e; bound %.2e %.2e" % ((name,) + e2 + bound))
        if name == "dw":
            assert e2[0] > 5 * bound[0] and e2[1] > 5 * bound[1], (name, e2, bound)
