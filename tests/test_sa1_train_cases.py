"""tests/sa1_train_cases.py checks itself on the CPU: the shape table's arithmetic, the conditions on every
row's seeded inputs, the mirror of the first layer's slice count, that the truth is the reference's module,
that finalize64 is the pooled variance, and that the bound of the GPU test (three times plain fp32's own
error plus the format's floor) passes the six partial products mlp_frag.h keeps and fails five of them."""
import pytest
import torch

import sa1_train_cases as C

ROWS = [(s[2], s[3], s[1]) for s in C.CHAIN_SHAPES]   # (b, m, ns)


def test_shape_table():
    assert len(set(ROWS)) == len(ROWS) == 12
    for case, ns, b, m, tpc, wgs, seed, momentum, running in C.CHAIN_SHAPES:
        assert C.chain_gate(b, m, ns) and (m * ns) % 256 == 0 and ns in (16, 32, 64)
        assert C.chain_arith(b, m, ns) == (tpc, wgs)
        assert wgs == b * m * ns // C.COLS_PER_PART
    by_case = {}
    for s in C.CHAIN_SHAPES:
        by_case.setdefault(s[0], []).append(s)
    assert all(sorted(s[1] for s in rows) == [16, 32, 64] for rows in by_case.values())
    assert all(s[5] == 1 for s in by_case["one_wg"])
    assert all(s[5] == 3 and s[2] == 3 for s in by_case["one_wg_b3"])          # three clouds of one workgroup
    assert all(s[5] == 6 and s[2] == 2 for s in by_case["three_wg"])           # three workgroups per cloud
    assert all(s[3] % C.TIE_EVERY == 0 for s in by_case["sevenths"])
    for s in by_case["sevenths"]:
        # the tied groups 0, 7, 14, ... of a cloud take every position a group can have in a workgroup
        ns, m = s[1], s[3]
        per_wg = C.COLS_PER_PART // ns
        assert {j % per_wg for j in range(0, m, C.TIE_EVERY)} == set(range(per_wg))
    # one row per ns at the other momentum, one row without running buffers
    assert sorted(s[1] for s in C.CHAIN_SHAPES if s[7] == 0.37) == [16, 32, 64]
    assert sum(1 for s in C.CHAIN_SHAPES if not s[8]) == 1
    assert not C.chain_gate(1, 8, 16) and not C.chain_gate(1, 32, 8) and not C.chain_gate(0, 16, 16)
    # the +30 channels of layer 1: one per (k step of 16, half of 8) corner
    assert {(c // 16, (c % 16) // 8) for c in C.BIG_CH_LIN4} == {(0, 0), (1, 0), (2, 1), (3, 1)}


@pytest.mark.parametrize("case,ns,b,m,tpc,wgs,seed,momentum,running", C.CHAIN_SHAPES)
def test_seeded_inputs_meet_their_conditions(case, ns, b, m, tpc, wgs, seed, momentum, running):
    inp = C.make_chain_inputs(b, m, ns, seed, momentum, running)
    info = C.check_inputs(inp, C.truth64(inp))
    print("%s ns %d: offsets %s %s, near-tied groups %.4f" % (case, ns, info["offset2"], info["offset3"], info["share"]))
    assert float((inp["sc0"] < 0).float().mean()) > 0.05
    assert bool((inp["g1"][::5] < 0).all()) and bool((inp["g2"][::5] < 0).all())
    assert int((inp["g1"] < 0).sum()) == 13 and int((inp["g2"] < 0).sum()) == 26
    assert float(inp["g2"][C.GAMMA2_ZERO_CH]) == 0.0
    assert not bool(inp["w1"][C.ZERO_ROW1].any()) and not bool(inp["w2"][C.ZERO_ROW2].any())
    if ns == 16:
        js = C.border_groups(m, ns)
        assert js and all(j % 2 == 0 for j in js)   # both groups inside one tile
    # the tied columns are the first of their value: the later copy never is the float64 arg-max
    _, first = C.first_winner(C.truth64(inp)["y3"], inp["g2"])
    for _, later in C.TIES + ((C.TIE_64,) if ns == 64 else ()):
        assert not bool((first[:, :, ::C.TIE_EVERY] == later).any())


def test_first4_slices_mirror():
    assert set(C.FIRST4_SLICES) == set(C.FIRST4_SHAPES)
    for shape, want in C.FIRST4_SLICES.items():
        assert C.first4_slices(*shape) == want, shape
        assert shape[1] % 4 == 0
    slices, per = C.first4_slices(1, 131076)
    assert 131076 - (slices - 1) * per == 4          # the last slice holds 4 columns
    assert C.first4_slices(600, 8)[0] == 1 and 600 > 512
    assert sorted(b * r for b, r in C.MOMENT_SHAPES[:-1]) == [1, 255, 256, 257, 65535, 65536, 65537]


@pytest.mark.parametrize("b,r", [s for s in C.FIRST4_SHAPES if s[0] * s[1] <= 4096])
@pytest.mark.parametrize("training", [True, False])
def test_first4_inputs_and_truth(b, r, training):
    """the inputs meet their conditions, the float64 autograd is the module's, and the formula the kernels
    use (dy = a (g - c1 - xhat c2)) in fp32 is fp32-grade against it"""
    inp = C.make_first4_inputs(b, r, training)
    C.check_first4_inputs(inp)
    truth = C.first4_truth64(inp)
    conv = torch.nn.Conv1d(4, 64, 1, bias=False).double()
    conv.weight.data.copy_(inp["w"].double().view(64, 4, 1))
    bn = torch.nn.BatchNorm1d(64, eps=C.EPS).double()
    bn.weight.data.copy_(inp["gamma"].double())
    bn.bias.data.copy_(inp["beta"].double())
    if training:
        bn.train()
    else:
        bn.eval()
        bn.running_mean.copy_(inp["mean"].double())
        bn.running_var.copy_(1.0 / inp["invstd"].double() ** 2 - C.EPS)
    (torch.relu(bn(conv(inp["x"].double()))) * inp["dz"].double()).sum().backward()
    assert torch.allclose(truth, conv.weight.grad.view(64, 4), rtol=0, atol=1e-9 * truth.abs().max().item())
    e32 = C.grad_errors(C.first4_plain_fp32(inp), truth)
    assert max(e32) < 1e-4, e32


@pytest.mark.parametrize("b,m,ns", [(1, 8, 32), (2, 12, 64)])
def test_truth_is_the_module(b, m, ns):
    inp = C.make_chain_inputs(b, m, ns, 0)
    tru = C.truth64(inp)
    a0 = torch.relu(torch.einsum("oc,bcmn->bomn", inp["w0"].double(), inp["x4"].double())
                    * inp["sc0"].double().view(1, -1, 1, 1) + inp["sh0"].double().view(1, -1, 1, 1))
    x = a0
    for layer, (w, g, be, rm, rv) in ((2, ("w1", "g1", "be1", "rm1", "rv1")), (3, ("w2", "g2", "be2", "rm2", "rv2"))):
        c_out, c_in = inp[w].shape
        conv = torch.nn.Conv2d(c_in, c_out, 1, bias=False).double()
        conv.weight.data.copy_(inp[w].double().view(c_out, c_in, 1, 1))
        bn = torch.nn.BatchNorm2d(c_out, eps=inp["eps"], momentum=inp["momentum"]).double().train()
        bn.weight.data.copy_(inp[g].double())
        bn.bias.data.copy_(inp[be].double())
        bn.running_mean.copy_(inp[rm].double())
        bn.running_var.copy_(inp[rv].double())
        y = conv(x)
        assert torch.allclose(y, tru["y%d" % layer], rtol=0, atol=1e-12 * y.abs().max().item())
        x = torch.relu(bn(y))
        run = tru["running%d" % layer]
        assert torch.allclose(bn.running_mean, run[0], rtol=1e-12, atol=1e-13)
        assert torch.allclose(bn.running_var, run[1], rtol=1e-12, atol=1e-13)
    pooled = torch.nn.functional.max_pool2d(x, kernel_size=[1, ns]).squeeze(-1)
    assert torch.allclose(pooled, tru["pooled"], rtol=0, atol=1e-11 * pooled.abs().max().item())
    # the gamma2 == 0 channel and the constant channel: relu(beta2)
    for ch in (C.GAMMA2_ZERO_CH, C.ZERO_ROW2):
        assert bool((tru["pooled"][:, ch] == torch.relu(inp["be2"][ch].double())).all())


def test_finalize64_is_the_pooled_variance():
    g = torch.Generator().manual_seed(5)
    y = torch.randn(3, 7, 40, 16, generator=g).double() * 2 + 5
    parts = y.permute(1, 0, 2, 3).reshape(7, 15, 128)        # 15 parts of 128 columns per channel
    pairs = torch.stack([parts.mean(2), ((parts - parts.mean(2, keepdim=True)) ** 2).sum(2)], dim=2).permute(1, 0, 2)
    gamma, beta = torch.rand(7, generator=g) + 0.5, torch.randn(7, generator=g)
    rm, rv = torch.randn(7, generator=g), torch.rand(7, generator=g) + 0.5
    got = C.finalize64(pairs, 128, gamma, beta, C.EPS, 0.37, rm, rv)
    st = C.stats_of(y, gamma, beta, C.EPS, torch.float64)
    for k in ("mean", "var", "invstd", "scale", "shift"):
        assert torch.allclose(got[k], st[k], rtol=1e-12, atol=1e-13), k
    n = 15 * 128
    assert torch.allclose(got["running_var"], 0.63 * rv.double() + 0.37 * st["var"] * n / (n - 1), rtol=1e-12)
    assert torch.allclose(got["running_mean"], 0.63 * rm.double() + 0.37 * st["mean"], rtol=1e-12)


@pytest.mark.parametrize("b,m,ns", [(s[2], s[3], s[1]) for s in C.CHAIN_SHAPES if s[0] in ("one_wg", "three_wg")])
def test_bound_fails_a_broken_split(b, m, ns):
    """split_form64 -- the chain as the kernels evaluate it, each GEMM the sum of partial products of the
    operands' bf16 terms -- under the GPU test's rule: with the six products mfma6 keeps it passes in every
    measure (both raw outputs globally and per channel, both layers' mean, invstd, scale and shift); with
    hi x lo deleted, and with mid x mid deleted, it FAILS in every measure.  The whole-tensor 2e-5 of
    tests/test_gpu_mlp.py sees neither (1.2e-5 - 3.6e-5 of the largest element)."""
    row = [s for s in C.CHAIN_SHAPES if (s[2], s[3], s[1]) == (b, m, ns)][0]
    inp = C.make_chain_inputs(b, m, ns, row[6], row[7], row[8])
    tru, p32 = C.truth64(inp), C.plain_fp32(inp)
    full = C.compare_chain(C.split_form64(inp, C.SIX), p32, tru, inp)
    assert len(full) == 12
    for name, ok, need, e, e32 in full:
        print("six products   %-12s %.2e (plain fp32 %.2e): %.2f of the bound" % (name, e, e32, need))
        assert ok, (name, e, e32)
    for what, gone in (("hi x lo", C.HI_LO), ("mid x mid", C.MID_MID)):
        rows = C.compare_chain(C.split_form64(inp, [p for p in C.SIX if p != gone]), p32, tru, inp)
        for name, ok, need, e, e32 in rows:
            print("without %-9s %-12s %.2e (plain fp32 %.2e): %.1f times the bound" % (what, name, e, e32, need))
            assert not ok, (what, name, e, e32, need)
        # ... and inside or at the edge of the old whole-tensor tolerance
        assert max(r[3] for r in rows if r[0].endswith("global")) < 4e-5
