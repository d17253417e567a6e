"""tests/pool_fwd256_cases.py checks itself on the CPU: the mirror of the range split gives the hand-computed
figures, the table reaches every edge of the persistent kernel's ranges at 256 CUs, the seeded inputs meet
their conditions on every row (whole rows: the largest takes about a second), the planted pairs sit where
the lane layout says, no tie assertion is vacuous, the float64 truth is the reference's module, and the
bound of the GPU test is tight enough to fail a kernel that drops one of its six partial products."""
import importlib

import pytest
import torch

from conftest import load_pkg
import pool_fwd256_cases as C

ROWS = [c[:3] for c in C.CASES]

# (b, groups, ns): blocks, grid, per, empty ranges, lengths of the others, crossing ranges -- by hand, 256 CUs
LISTED = {
    (1, 8, 32): (2, 2, 1, 0, {1}, 0), (1, 16, 16): (2, 2, 1, 0, {1}, 0),
    (3, 8, 32): (6, 6, 1, 0, {1}, 0), (3, 16, 16): (6, 6, 1, 0, {1}, 0),
    (2, 136, 32): (68, 68, 1, 0, {1}, 0),
    (129, 8, 32): (258, 256, 2, 127, {2}, 0), (1, 2064, 16): (258, 256, 2, 127, {2}, 0),
    (257, 8, 32): (514, 256, 3, 84, {1, 3}, 171), (257, 16, 16): (514, 256, 3, 84, {1, 3}, 171),
    (7, 296, 32): (518, 256, 3, 83, {2, 3}, 4), (37, 112, 16): (518, 256, 3, 83, {2, 3}, 24),
    (5, 1232, 16): (770, 256, 4, 63, {2, 4}, 2),
}


def test_split_partitions_the_blocks():
    for cus in (1, 3, 104, 256, 304):
        for blocks in list(range(1, 800)) + [2048, 8192]:
            grid, per, ranges = C.split(blocks, cus)
            assert grid == min(cus, blocks) and len(ranges) == grid
            at = 0
            for lo, hi in ranges:   # in order, without gaps; what is left over is empty ranges at the end
                if lo < hi:
                    assert lo == at and hi - lo <= per
                    at = hi
                else:
                    assert at == blocks
            assert at == blocks


def test_listed_figures():
    assert set(ROWS) == set(LISTED) and len(ROWS) == len(set(ROWS))
    for row in ROWS:
        d = C.describe(*row)
        assert (d["blocks"], d["grid"], d["per"], d["empty"], d["lengths"], d["crossing"]) == LISTED[row], row
    # every cloud of (257, *, *) is two blocks: each range of three meets a boundary at one of two positions
    for row in ((257, 8, 32), (257, 16, 16)):
        assert C.describe(*row)["offsets"] == {1, 2}
    # the last range of the rows with a short one is the only short one
    for row, short in (((257, 8, 32), 1), ((7, 296, 32), 2), ((37, 112, 16), 2), ((5, 1232, 16), 2)):
        live = [hi - lo for lo, hi in C.split(C.describe(*row)["blocks"])[2] if lo < hi]
        assert live[-1] == short and all(n == live[0] for n in live[:-1]) and live[0] > short


def test_table_reaches_every_edge():
    reached = C.edges(ROWS)
    assert reached >= C.EDGES, C.EDGES - reached
    ds = {row: C.describe(*row) for row in ROWS}
    assert {d["per"] for d in ds.values()} == {1, 2, 3, 4}
    lengths = set().union(*[d["lengths"] for d in ds.values()])
    assert lengths == {1, 2, 3, 4} and {4 * n % 3 for n in lengths} == {0, 1, 2}
    assert any(d["empty"] for d in ds.values())
    for ns in (16, 32):
        mine = [d for (_, _, n), d in ds.items() if n == ns]
        assert len(set().union(*[d["offsets"] for d in mine])) > 1 and any(d["crossing"] for d in mine)
        assert any(d["blocks"] == 2 and d["grid"] == 2 and d["per"] == 1 for d in mine)
    # a device with another CU count does not reach them all: the GPU test recomputes and fails there
    assert not C.edges(ROWS, 304) >= C.EDGES


def test_rows_are_covered_and_small():
    for b, groups, ns in ROWS:
        r = groups * ns
        assert C.covers(b, C.M_OUT, C.K_IN, r, ns) and r % 256 == 0
        assert b * C.K_IN * r * 4 <= 51e6            # y2, bytes
        assert b * C.M_OUT * r * 8 * 4 < 1e9         # the float64 y3 and its kin; a handful are alive at once
    b, groups, ns = C.TILED_EXTRA[:3]
    assert ns == 64 and not C.covers(b, C.M_OUT, C.K_IN, groups * ns, ns)
    assert C.stats_pool_supported(b, C.M_OUT, C.K_IN, groups * ns, ns)


@pytest.mark.parametrize("ns", [16, 32, 64])
def test_planted_pairs_sit_where_the_layout_says(ns):
    (a0, a1), (b0, b1), (c0, c1), (d0, d1) = C.tie_pairs(ns)
    assert all(0 <= k < l < ns for k, l in C.tie_pairs(ns))
    assert len({n for pair in C.tie_pairs(ns) for n in pair}) == 8   # no column in two pairs
    if ns == 64:
        return   # (the tiled kernel alone: no half-waves of this layout)
    slot = lambda n: C.lane_slot(n, ns)  # noqa: E731
    # the MFMA's 32 x 32 accumulator: register q of half-wave h holds row (q & 3) + 8 (q >> 2) + 4 h
    for n in range(ns):
        h, q, upper = slot(n)
        assert (q & 3) + 8 * (q >> 2) + 4 * h == n and upper == (q >= ns // 4)
    assert slot(a0)[0] == slot(a1)[0] and slot(a0)[2] == slot(a1)[2]            # same half-wave, same half
    assert slot(b0)[0] == slot(b1)[0] and (slot(b0)[2], slot(b1)[2]) == (False, True)   # lower against upper half
    assert (slot(c0)[0], slot(c1)[0]) == (0, 1)      # across, the earlier sample in the lower half-wave
    assert (slot(d0)[0], slot(d1)[0]) == (1, 0)      # across, the earlier sample in the upper half-wave
    dup = C.later_copies(8, ns)
    assert int(dup.sum()) == 8 and all(bool(dup[cls, later]) and bool(dup[cls + 4, later])
                                       for cls, (_, later) in enumerate(C.tie_pairs(ns)))


@pytest.mark.parametrize("b,groups,ns,seed", C.CASES + (C.TILED_EXTRA,))
def test_seeded_inputs_meet_their_conditions(b, groups, ns, seed):
    inp = C.make_inputs(b, groups, ns, seed)
    tru = C.truth64(inp)
    info = C.check_inputs(inp, tru)
    assert info["share"] <= C.MAX_EXCLUDED and min(info["offset"]) >= C.MIN_OFFSET_RATIO
    g3 = inp["gamma3"]
    assert int((g3 < 0).sum()) == 52 and bool((g3[::5] < 0).all())
    assert float(g3[C.GAMMA3_ZERO_CH]) == 0.0 and float(g3[C.GAMMA3_NEGZERO_CH]) == 0.0
    assert bool(torch.signbit(g3[C.GAMMA3_NEGZERO_CH])) and not bool(torch.signbit(g3[C.GAMMA3_ZERO_CH]))
    assert int((inp["scale"] < 0).sum()) >= 26   # every fifth gamma of the input layer, and one +30 channel
    # OFFSET_ROWS: different waves, both halves of a half-wave's lanes, both signs of gamma3
    rows = [row for row, _ in C.OFFSET_ROWS]
    assert len({row // 32 for row in rows}) >= 3 and {(row % 32) // 16 for row in rows} == {0, 1}
    assert {bool(g3[row] < 0) for row in rows} == {False, True}
    # no tie assertion is vacuous: each pair's kept column wins somewhere, and the copy never does
    idx = tru["idx"]
    assert int(idx.min()) >= 0 and int(idx.max()) < ns
    for cls, (kept, later) in enumerate(C.tie_pairs(ns)):
        assert bool((idx[:, :, cls::4] == kept).any()), (cls, kept)
        assert not bool((idx[:, :, cls::4] == later).any())
        others = [c for c in range(4) if c != cls]
        assert any(bool((idx[:, :, c::4] == later).any()) for c in others)   # (where it is no copy it can win)
    assert bool((idx[:, C.ZERO_ROW] == 0).all()) and bool((tru["win"][:, C.ZERO_ROW] == 0).all())


def test_truth_is_the_module():
    """Conv2d 1x1 without bias / BatchNorm2d on batch statistics / ReLU / max over nsample in float64"""
    b, groups, ns, seed = C.CASES[2]
    inp = C.make_inputs(b, groups, ns, seed)
    tru = C.truth64(inp)
    conv = torch.nn.Conv2d(C.K_IN, C.M_OUT, 1, bias=False).double()
    conv.weight.data.copy_(inp["w3"].double().view(C.M_OUT, C.K_IN, 1, 1))
    bn = torch.nn.BatchNorm2d(C.M_OUT, eps=C.EPS).double().train()
    bn.weight.data.copy_(inp["gamma3"].double())
    bn.bias.data.copy_(inp["beta3"].double())
    a2 = torch.relu(inp["y2"].double() * inp["scale"].double().view(1, -1, 1, 1) + inp["shift"].double().view(1, -1, 1, 1))
    with torch.no_grad():
        y3 = conv(a2)
        pooled = torch.nn.functional.max_pool2d(torch.relu(bn(y3)), kernel_size=[1, ns]).squeeze(-1)
    assert torch.allclose(y3, tru["y3"], rtol=0, atol=1e-12 * float(y3.abs().max()))
    st = tru["stats"]
    mine = torch.relu(tru["win"] * st["scale"].view(1, -1, 1) + st["shift"].view(1, -1, 1))
    assert torch.allclose(mine, pooled, rtol=0, atol=1e-11 * float(pooled.abs().max()))
    # the per-tile pairs finalize to the batch statistics (equal counts: the pooled-variance formula)
    fin = C.finalize64(tru["pairs"], C.TILE, inp["gamma3"], inp["beta3"], inp["eps"], inp["momentum"])
    assert torch.allclose(fin["mean"], st["mean"], rtol=0, atol=1e-12 * float(st["mean"].abs().max()))
    assert torch.allclose(fin["var"], st["var"], rtol=1e-11, atol=0)
    # and plain fp32 is fp32-grade
    p32 = C.plain_fp32(inp)
    assert C.tensor_errors(p32["y3"], tru["y3"], st["var"])[0] < 2e-6


FIVE = {"without hi x lo": [p for p in C.SIX if p != C.HI_LO], "without lo x hi": [p for p in C.SIX if p != (0, 2)]}


@pytest.mark.parametrize("row", [2, 3, 4])
def test_bound_fails_a_dropped_partial_product(row):
    """The six-product form is closer to the truth than a five-product one, and the five-product one misses the
    GPU test's bound on y (RATIO x plain fp32 + one ulp of the range, global and per channel) while the six-
    product one is far inside it.  Measured, need = error / bound, (global, worst channel):
      row            plain fp32 error    six             without hi x lo (PF_MM1(hi, lo))   without lo x hi
      (3, 8, 32)     6.1e-7, 3.7e-5      0.04, 0.04      4.06, 3.87  (7.9e-6 of the range)    7.82, 7.96
      (3, 16, 16)    5.7e-7, 3.1e-5      0.04, 0.04      2.12, 2.42  (3.9e-6)                 8.10, 8.47
      (2, 136, 32)   7.8e-7, 4.6e-5      0.03, 0.03      1.80, 1.93  (4.5e-6)                 6.20, 6.33
    (The fixed 2e-6 x range of test_gpu_mlp.py is missed by the five-product forms too, by a factor 2 to 4.)"""
    b, groups, ns, seed = C.CASES[row]
    inp = C.make_inputs(b, groups, ns, seed)
    tru, p32 = C.truth64(inp), C.plain_fp32(inp)
    var = tru["stats"]["var"]
    pg, pc = C.tensor_errors(p32["y3"], tru["y3"], var)
    fg, fc = C.tensor_floors(tru["y3"], var)

    def needs(products):
        y = C.split_form64(inp, products).float()   # (the accumulator is fp32)
        eg, ec = C.tensor_errors(y, tru["y3"], var)
        return C.within(eg, pg, fg)[1], C.within(ec, pc, fc)[1], eg

    six = needs(C.SIX)
    print("six products: need %.2f global, %.2f per channel; error %.2e" % six)
    assert six[0] < 0.25 and six[1] < 0.25
    for name, products in FIVE.items():
        five = needs(products)
        print("%s: need %.2f global, %.2f per channel; error %.2e" % ((name,) + five))
        assert five[0] > 1 and five[1] > 1, (name, five)
        assert five[2] > 10 * six[2]


def test_covers_agrees_with_the_library(monkeypatch):
    """covers == mlp_gemm_forward_stats_pool_supported and the kernel's own rule ((256, 128), nsample 16 / 32,
    whole 256-column blocks), asked of the library's host side (no GPU needed: shape gates only)"""
    try:
        load_pkg()
        lib = importlib.import_module("pointnet2._mlp_ext")._lib
    except (ImportError, OSError) as e:   # no host build on this machine
        pytest.skip("the library does not load here: %s" % e)
    monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "0")
    seen = set()
    for b in (0, 1, 3):
        for m, k in ((256, 128), (128, 128), (256, 64), (256, 130), (64, 128)):
            for r in (0, 128, 256, 384, 512, 768, 1000, 1024):
                for ns in (8, 16, 32, 64, 48):
                    entry = bool(lib.mlp_gemm_forward_stats_pool_supported(b, m, k, r, ns))
                    assert entry == C.stats_pool_supported(b, m, k, r, ns), (b, m, k, r, ns)
                    mine = C.covers(b, m, k, r, ns)
                    assert mine == (entry and (m, k) == (C.M_OUT, C.K_IN) and ns in (16, 32)), (b, m, k, r, ns)
                    seen.add((entry, mine))
    assert seen == {(False, False), (True, False), (True, True)}
    # the small-layer threshold moves the entry point's answer, not the mirror's
    monkeypatch.setenv("MLP_SMALL_GEMM_COLS", "16384")
    assert not lib.mlp_gemm_forward_stats_pool_supported(1, 256, 128, 256, 32)
    assert C.stats_pool_supported(1, 256, 128, 256, 32, small_cols=16384) is False
    assert lib.mlp_gemm_forward_stats_pool_supported(65, 256, 128, 256, 32)
