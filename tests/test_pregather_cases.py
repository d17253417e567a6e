"""tests/pregather_cases.py checks itself on the CPU: the shape table against the restated gate and the
kernels' arithmetic, that the index rows between them hold every class of run the backward kernel stitches,
the conditions on every row's seeded inputs, and that the rule of the GPU test (three times plain fp32's own
error plus the derived floor) passes the kernels' algebra evaluated in fp32 on the CPU and fails it with a
sign, a swapped coefficient or a dropped partial sum."""
import functools

import pytest
import torch

import pregather_cases as C

IDS = [C.row_id(r) for r in C.INDEX_ROWS]
OVER = (1, 2)                 # the backward's yardstick: plain fp32's worst figure of the cloud


@functools.lru_cache(maxsize=None)
def _census(row):
    case, b, c, n, m, ns, pats = row
    idx = C.make_idx(row)
    return [C.census(idx[i], n) for i in range(b)]


def test_shape_table():
    assert [s[0] for s in C.SHAPES] == list(C.SHAPE_CHUNK)
    for case, b, c, n, m, ns in C.SHAPES:
        assert C.gate(b, c, n, m, ns), case
        assert c % 4 == 0 and n <= 4096 and m <= 4096 and ns >= 4 and ns & (ns - 1) == 0 and m * ns <= 32768
        assert C.chunk(m * ns) == C.SHAPE_CHUNK[case]
    by = {s[0]: s[1:] for s in C.SHAPES}
    assert by["one_quad"][2:] == (1, 1, 4) and C.index_loads(4) == (1, 1)
    assert C.forward_workgroups(*by["nine_wgs"][:2]) == 9 and 9 % 8 != 0
    b, c, n, m, ns = by["pad_mid_lane"]
    assert m * ns == 5004 and 5004 % 8 != 0 and C.index_loads(5004) == (2, 1251 - 1024)
    b, c, n, m, ns = by["no_pad"]
    assert m * ns == 4 * C.THREADS
    b, c, n, m, ns = by["limits"]
    assert (n, m, m * ns) == (C.MAX_POINTS, C.MAX_GROUPS, C.MAX_ENTRIES) and C.index_loads(m * ns) == (8, 1024)
    assert by["wide_groups"][4] == 128 and by["wide_groups"][2] == 3
    assert {C.chunk(s[4] * s[5]) for s in C.SHAPES} == {4, 8, 16, 32}
    # just outside: one condition each
    assert len(C.OUTSIDE) == 6
    for what, b, c, n, m, ns in C.OUTSIDE:
        assert not C.gate(b, c, n, m, ns), what
    assert C.OUTSIDE[5][4] * C.OUTSIDE[5][5] == 32768 + 4 * C.OUTSIDE[5][5]
    assert not C.gate(0, 4, 1, 1, 4) and not C.gate(1, 0, 1, 1, 4) and C.gate(1, 4, 4096, 4096, 8)
    # pack / unpack beside the table: n + m and n off a multiple of 256
    assert any((n + m) % 256 and n % 256 for _, _, n, m in C.pack_shapes())
    assert {(n + m) % 256 for _, _, n, m in C.PACK_SHAPES} >= {0, 1, 255}


def test_index_rows_cover_every_pattern():
    rows = {}
    for row in C.INDEX_ROWS:
        assert len(row[6]) == row[1]
        rows.setdefault(row[0], set()).update(row[6])
    for case, b, c, n, m, ns in C.SHAPES:
        assert rows[case] == {p for p in C.PATTERNS if C.pattern_ok(p, n, m, ns)}, case
        assert {"ball", "one_point"} <= rows[case]
    assert rows["nine_wgs"] == set(C.PATTERNS)                  # the one shape with m ns <= n
    assert "lane_runs" in rows["limits"] and "lane_runs_shifted" in rows["sa3"]
    assert "lane_runs" not in rows["wide_groups"]               # three points cannot fill 800 lanes once each


@pytest.mark.parametrize("row", C.INDEX_ROWS, ids=IDS)
def test_patterns_are_what_they_say(row):
    case, b, c, n, m, ns, pats = row
    idx = C.make_idx(row)
    ch = C.chunk(m * ns)
    for i, p in enumerate(pats):
        flat = idx[i].reshape(-1).long()
        counts = torch.bincount(flat, minlength=n)
        used = counts[counts > 0]
        cen = _census(row)[i]
        if p == "ball":
            assert int(flat.max()) < max(1, 3 * n // 4)
            assert torch.equal(idx[i][:, ns // 2:], idx[i][:, :1].expand(m, ns - ns // 2))
        elif p == "one_point":
            assert bool((flat == n - 1).all()) and cen["g_one_run"] == 1
        elif p == "two_alternating":
            quads = flat.view(-1, 4)
            assert bool((quads[:, 1:] != quads[:, :-1]).all()) and used.numel() == 2
        elif p == "each_once":
            assert bool((used == 1).all())
        elif p == "lane_runs":
            assert bool((used[:-1] == ch).all()) and 0 < int(used[-1]) <= ch
            assert cen["b_one_boundary"] == cen["c_middle_lane"] == 0   # every run inside its lane
        elif p == "lane_runs_shifted":
            assert int(used[0]) == 1 and bool((used[1:-1] == ch).all()) and int(used[-1]) <= 2 * ch - 1
            if used.numel() > 2:
                assert cen["a_inside_lane"] <= 2 and cen["b_one_boundary"] >= used.numel() - 3


def test_census_shows_every_class():
    where = {k: [] for k in C.CLASSES}
    for row in C.INDEX_ROWS:
        for i, cen in enumerate(_census(row)):
            assert set(cen) == set(C.CLASSES)
            for k, v in cen.items():
                if v >= 1:
                    where[k].append("%s[%d: %s]" % (row[0], i, row[6][i]))
    for k in C.CLASSES:
        print("%-22s %d clouds, e.g. %s" % (k, len(where[k]), ", ".join(where[k][:3])))
    for k in C.CLASSES:
        assert where[k], "no cloud of the table shows class %s" % k
    # and where each is expected
    has = lambda k, case, pat: any(w.startswith(case + "[") and w.endswith(pat + "]") for w in where[k])  # noqa: E731
    assert has("a_inside_lane", "sa3", "lane_runs"), where["a_inside_lane"]
    assert has("b_one_boundary", "sa3", "lane_runs_shifted"), where["b_one_boundary"]
    assert has("c_middle_lane", "wide_groups", "two_alternating"), where["c_middle_lane"]
    assert has("d_wave_boundary", "limits", "lane_runs_shifted"), where["d_wave_boundary"]
    assert has("e_ends_with_lane", "limits", "lane_runs"), where["e_ends_with_lane"]
    assert has("f_pad_same_lane", "pad_mid_lane", "ball"), where["f_pad_same_lane"]
    assert has("f_pad_next_lane", "nine_wgs", "ball"), where["f_pad_next_lane"]
    assert has("f_no_pad", "no_pad", "ball"), where["f_no_pad"]
    assert has("g_one_run", "limits", "one_point"), where["g_one_run"]
    assert has("h_unreferenced", "sa3", "ball") and has("h_point_last", "sa3", "ball"), where["h_point_last"]
    assert has("h_point_0", "limits", "lane_runs"), where["h_point_0"]
    for k in ("i_lane_1023_live", "i_lane_1023_covered", "i_lane_1023_continued"):
        assert has(k, "no_pad", "one_point") and has(k, "limits", "one_point"), where[k]


def test_census_by_hand():
    # 8 entries, CHUNK 4 (two live lanes): keys sorted 0 0 0 | 2 2 2 2 | 5 -> lanes [0 0 0 2] [2 2 2 5]
    cen = C.census(torch.tensor([2, 0, 2, 5, 0, 2, 0, 2]), 7)
    assert (cen["a_inside_lane"], cen["b_one_boundary"], cen["c_middle_lane"]) == (2, 1, 0)
    assert cen["e_ends_with_lane"] == 0 and cen["f_pad_next_lane"] == 1 and cen["h_unreferenced"] == 4
    assert cen["h_point_0"] == 0 and cen["h_point_last"] == 1 and cen["i_lane_1023_live"] == 0
    # twelve entries of one key and four of another: lanes [1 1 1 1] [1 1 1 1] [1 1 1 1] [3 3 3 3]
    cen = C.census(torch.tensor([1] * 12 + [3] * 4), 4)
    assert (cen["a_inside_lane"], cen["b_one_boundary"], cen["c_middle_lane"]) == (1, 0, 1)
    assert cen["e_ends_with_lane"] == 1 and cen["d_wave_boundary"] == 0 and cen["g_one_run"] == 0
    # 4096 entries, CHUNK 4, one key over lanes 63 .. 64 and one over the last two lanes
    keys = torch.arange(1024).repeat_interleave(4)
    keys[63 * 4:65 * 4] = 63
    keys[1022 * 4:] = 1022
    cen = C.census(keys[torch.randperm(4096, generator=torch.Generator().manual_seed(0))], 1024)
    assert cen["d_wave_boundary"] == 1 and cen["b_one_boundary"] == 2 and cen["f_no_pad"] == 1
    assert (cen["i_lane_1023_live"], cen["i_lane_1023_covered"], cen["i_lane_1023_continued"]) == (1, 1, 1)


@pytest.mark.parametrize("row", C.INDEX_ROWS, ids=IDS)
def test_seeded_inputs_meet_their_conditions(row):
    info = C.check_inputs(row)
    print("%s: outlier %.1f sigma, %d constant rows" % (C.row_id(row), info["outlier"], info["constant_rows"]))
    assert info["constant_rows"] >= row[1]


def test_outlier_rows_reach_six_sigma():
    best = {C.row_id(r): C.check_inputs(r)["outlier"] for r in C.INDEX_ROWS if r[0] in ("sa3", "pad_mid_lane")}
    assert max(best.values()) >= C.MIN_OUTLIER, best
    assert best["sa3-ball+one_point"] >= C.MIN_OUTLIER, best


def test_pack_truth_layout():
    xyz, new_xyz, feat = C.make_pack_inputs(2, 3, 5, 2)
    out = C.pack_truth(xyz, new_xyz, feat, 1.25)
    assert tuple(out.shape) == (2, 6, 7)
    assert float(out[1, 2, 4]) == float(xyz[1, 4, 2] * 1.25) and float(out[0, 0, 6]) == float(new_xyz[0, 1, 0] * 1.25)
    assert torch.equal(out[:, 3:, :5], feat) and not bool(out[:, 3:, 5:].any())
    assert torch.equal(C.unpack_truth(out, 5), feat)


@pytest.mark.parametrize("row", C.INDEX_ROWS, ids=IDS)
def test_pair_rule_on_the_cpu(row):
    """the yardstick and the kernel's shifted-sum form, both in fp32 torch, are within the rule against float64;
    a mean that takes its shift from another element than the sums is not"""
    case, b, c, n, m, ns, pats = row
    inp = C.make_forward_inputs(row)
    y = C.forward_truth(inp["z"], inp["idx"], n)
    tru = C.pair_truth64(y)
    live = tru[1] > 0             # (on a constant row plain fp32's mean of equal numbers is not exact: pair_rule)
    for p, fl in zip(C.pair_errors(C.pair_plain_fp32(y), tru, m * ns), C.pair_floors(tru, m * ns)):
        assert bool(torch.isfinite(p[live]).all()) and (not bool(live.any()) or C.within(p[live], p[live], fl[live])[0])
    form = C.kernel_form_pairs(y)
    for name, ok, need, worst, worst32 in C.pair_rule(form, y):
        print("%s %-20s shifted form %.2e | plain fp32 %.2e | %.2f of the bound" % (C.row_id(row), name, worst, worst32, need))
        assert ok, (name, need)
    flat = y.flatten(2)
    if bool((flat[:, :, 0] != flat[:, :, 1]).any()):
        wrong = (form[0] - flat[:, :, 0] + flat[:, :, 1], form[1])
        assert not all(r[1] for r in C.pair_rule(wrong, y)[:2])


@pytest.mark.parametrize("row", C.INDEX_ROWS, ids=IDS)
def test_backward_truths_on_the_cpu(row):
    """exact form: the int64 truth is what float64 gives; general form: the yardstick and the folded form in
    fp32 are within the rule, the folded form with c1 and c2 swapped, with the group sums' sign lost or with one
    entry dropped is not"""
    case, b, c, n, m, ns, pats = row
    ex = C.make_exact_backward(row)
    want = C.exact_backward_truth(ex)
    assert want.dtype == torch.int64 and tuple(want.shape) == (b, c, n + m)
    assert int(want.abs().max()) < 2 ** 24
    gated = torch.where(ex["y"] > 0, ex["dz"], torch.zeros(())).double()
    assert torch.equal(want.double(), C._scatter(gated, ex["idx"], n))
    assert torch.equal(C.kernel_form_backward(ex).double(), want.double())      # the fold is exact on this data
    assert int(want[:, :, :n].sum()) == -int(want[:, :, n:].sum())
    gen = C.make_general_backward(row)
    truth, mass, floor_abs = C.general_backward_truth64(gen)
    floor = C.backward_floor(mass, floor_abs)
    assert float(floor.max()) <= 3.0001 * C.ULP, float(floor.max())             # a few ULP of the mass
    e32 = C.backward_errors(C.general_backward_plain_fp32(gen), truth, mass)
    assert bool(torch.isfinite(e32).all()) and float(e32.max()) <= 1e-3
    ok, need, worst, worst32 = C.within(C.backward_errors(C.kernel_form_backward(gen), truth, mass), e32, floor, OVER)
    print("%s folded form %.2e | plain fp32 %.2e | floor %.2e | %.2f of the bound"
          % (C.row_id(row), worst, worst32, float(floor.max()), need))
    assert ok, need
    for mutant in (C.kernel_form_backward(gen, swap_c=True), C.kernel_form_backward(gen, sign=1.0)):
        assert not C.within(C.backward_errors(mutant, truth, mass), e32, floor, OVER)[0]
    dropped = dict(gen)
    dropped["dz"] = gen["dz"].clone()
    live = C.open_gate(gen).flatten().nonzero()
    if live.numel():
        dropped["dz"].view(-1)[int(live[0])] = 0.0
        assert not C.within(C.backward_errors(C.kernel_form_backward(dropped), truth, mass), e32, floor, OVER)[0]
