"""Shapes, inputs, float64 truth and fp32 yardstick for the tests of the pooled 128 -> 256 forward
(csrc/mlp_pool_fwd256.hip: pool_fwd256_kernel<16|32, STORE>, and the tiled gemm_nn2_kernel with its
pooled epilogue behind the same entry point, mlp_gemm_forward_stats_pool); no package import.

The kernel is persistent.  A block is 4 chunks of 32 columns (two 64-column tiles); with
blocks = b * r / 128, grid = min(CUs, blocks) and per = ceil(blocks / grid), workgroup i owns the blocks
[i * per, min(i * per + per, blocks)).  A range may be empty, shorter than the others, and may run from
one cloud into the next; its length in chunks mod 3 decides where the ring of three LDS buffers ends.

Sample n of a group (ns = 16 / 32) sits in half-wave (n >> 2) & 1, register slot (n & 3) + 4 * (n >> 3)
of its group's registers; the upper half of the slots is scanned first, then the lower, then the two
half-waves are merged (pieces 14, 15, 18 of the kernel).

  covers(b, m, k, r, ns)          mlp_pool_fwd256_supported without the pointer alignment
  split(blocks, cus)              (grid, per, ranges) as the launch and the kernel compute them
  describe(b, groups, ns, cus)    what the ranges of a row of CASES look like
  edges(rows, cus)                the edge set the table has to reach (tests/test_pool_fwd256_cases.py
                                  proves it at 256 CUs, the GPU test asserts it at the device's count)
  CASES                           (b, groups, ns, seed); r = groups * ns, r % 256 == 0
  make_inputs(b, groups, ns, seed)   see its docstring; nothing of the project prepares an input
  truth64(inp)                    a2 = relu(y2 scale + shift), y3 = w3 a2 (conv 1x1 without bias,
                                  pytorch_utils.py:70-124) in float64 from the fp32 operands promoted; per tile
                                  of 64 columns and channel (mean, M2); the batch statistics; per group the
                                  winner under pool_sign(gamma3) and its first index
                                  (pointnet2_modules.py:256-262: BatchNorm and ReLU are monotone in y3)
  plain_fp32(inp)                 the same in fp32 torch ops with TF32 off, two-pass (mean, M2): the yardstick
  split_form64(inp, products)     the product in float64 from the operands' bf16 terms, keeping the listed
                                  partial products (default: the six the kernel issues)
  check_inputs(inp, tru)          the conditions on the data, asserted before anything is compared
  pair_errors / pair_floors / own_pair_floors / one_pass_floor, tile_pairs   the measures of the per-tile pairs
"""
import torch

from sa1_train_cases import (EPS, GATE_ULPS, MAX_EXCLUDED, MIN_OFFSET_RATIO, RATIO, SIX, ULP, WIN_ULPS,  # noqa: F401
                             _tf32_off, bf16_terms, finalize64, first_winner, pool_sign, stat_errors, stat_floors,
                             own_floors, stats_of, tensor_errors, tensor_floors, within)

K_IN, M_OUT, CHUNK, TILE, BLOCK = 128, 256, 32, 64, 128
CUS = 256                     # the CU count the table was laid out for
BIG_IN_CH = (6, 77)           # input channels with shift = +30 and a small scale (+0.05 / -0.05)
BIG_SHIFT, BIG_SCALE = 30.0, 0.05
SHUT_IN_CH = 40               # shift = -50: its ReLU is shut in every column
SHUT_SHIFT = -50.0
ZERO_ROW = 141                # all-zero row of w3: that output channel is the constant 0 (gamma3 > 0 there)
# rows with weight 1.0 on a +30 input channel: (row, input channel).  Waves 0, 1, 4, 7 (32 channels per
# wave), lanes 3 / 9 (lower sixteen of a half-wave) and 19 / 26 (upper); row 250 has a negative gamma3
OFFSET_ROWS = ((3, 6), (51, 77), (137, 6), (250, 77))
GAMMA3_ZERO_CH, GAMMA3_NEGZERO_CH = 33, 98   # gamma3 == 0.0 / -0.0: `gamma < 0` is false, the largest wins
MOMENTUM = 0.1
HI_LO = (2, 0)                # (weight term, activation term): the product PF_MM1(hi, lo) issues


def tie_pairs(ns):
    """(kept, later copy) per residue class of the group index mod 4"""
    return ((1, 3),               # same half-wave, same register half
            (2, ns // 2 + 1),     # same half-wave, lower against upper register half
            (0, ns - 1),          # across the half-waves, the earlier sample in the lower one
            (5, 8))               # across the half-waves, the earlier sample in the upper one


def lane_slot(n, ns):
    """sample n of a group -> (half-wave, register slot within the group's registers, upper half of them?)"""
    slot = (n & 3) + 4 * (n >> 3)
    return (n >> 2) & 1, slot, slot >= (ns // 2) // 2


# (b, groups, ns, seed).  The seeds are those at which check_inputs holds
# (tests/test_pool_fwd256_cases.py runs it on every row).
CASES = (
    (1, 8, 32, 0), (1, 16, 16, 0),         # 2 blocks: two workgroups, one block each
    (3, 8, 32, 0), (3, 16, 16, 0),         # 6 blocks, three clouds
    (2, 136, 32, 0),                       # 68 blocks, per = 1
    (129, 8, 32, 0), (1, 2064, 16, 2),     # 258 blocks, per = 2, 127 empty, no crossing
    (257, 8, 32, 0), (257, 16, 16, 5),     # 514, per = 3, 84 empty, lengths {3, 1}, 171 crossing
    (7, 296, 32, 0), (37, 112, 16, 2),     # 518, per = 3, 83 empty, last of 2; 4 / 24 crossing
    (5, 1232, 16, 2),                      # 770, per = 4, 63 empty, last of 2; 2 crossing
)
TILED_EXTRA = (2, 8, 64, 0)                # nsample 64: the tiled kernel only


# ------------------------------------------------------------------ the split
def covers(b, m, k, r, ns):
    """mlp_pool_fwd256_supported, the pointer alignment left out"""
    return b > 0 and m == M_OUT and k == K_IN and r > 0 and r % 256 == 0 and ns in (16, 32) and r % ns == 0


def stats_pool_supported(b, m, k, r, ns, small_cols=0):
    """mlp_gemm_forward_stats_pool_supported (mlp_gemm_forward_stats_parts > 0 inside it)"""
    if b <= 0 or r % 256 != 0 or b * r <= small_cols:
        return False
    if not (m == 256 or 32 < m <= 128):
        return False
    return m in (128, 256) and ns in (16, 32, 64) and r % ns == 0 and k % 4 == 0


def split(blocks, cus=CUS):
    """-> (grid, per, [(k_lo, k_hi)] * grid) in blocks"""
    grid = min(cus, blocks)
    per = (blocks + grid - 1) // grid
    return grid, per, [(i * per, min(i * per + per, blocks)) for i in range(grid)]


def describe(b, groups, ns, cus=CUS):
    """-> dict(blocks, grid, per, empty, lengths: set of the live ranges' lengths in blocks, crossing: live
    ranges whose blocks lie in more than one cloud, offsets: set of the positions (in blocks from the
    range's start) at which a live range meets a cloud boundary)"""
    per_cloud = groups * ns // BLOCK
    blocks = b * per_cloud
    grid, per, ranges = split(blocks, cus)
    live = [(lo, hi) for lo, hi in ranges if lo < hi]
    offsets = {k - lo for lo, hi in live for k in range(lo + 1, hi) if k % per_cloud == 0}
    return {"blocks": blocks, "grid": grid, "per": per, "empty": len(ranges) - len(live),
            "lengths": {hi - lo for lo, hi in live},
            "crossing": sum(1 for lo, hi in live if lo // per_cloud != (hi - 1) // per_cloud),
            "offsets": offsets}


def edges(rows, cus=CUS):
    """The edges of the range split that `rows` reach at `cus` CUs, as a set of names"""
    out = set()
    for ns in (16, 32):
        ds = [describe(b, g, n, cus) for b, g, n in rows if n == ns]
        out |= {"per %d" % d["per"] for d in ds} | {"length %d" % n for d in ds for n in d["lengths"]}
        out |= {"chunks mod 3 = %d" % (4 * n % 3) for d in ds for n in d["lengths"]}
        if any(d["empty"] for d in ds):
            out.add("empty")
        if any(d["blocks"] == 2 and d["grid"] == 2 for d in ds):
            out.add("two blocks ns %d" % ns)
        if any(d["crossing"] for d in ds):
            out.add("crossing ns %d" % ns)
        if len(set().union(*[d["offsets"] for d in ds])) > 1:
            out.add("crossing at two offsets ns %d" % ns)
        # a short last range behind full ones
        if any(len(d["lengths"]) > 1 for d in ds):
            out.add("short last range ns %d" % ns)
    return out


EDGES = ({"per %d" % p for p in (1, 2, 3, 4)} | {"length %d" % n for n in (1, 2, 3, 4)}
         | {"chunks mod 3 = %d" % q for q in (0, 1, 2)} | {"empty"}
         | {"%s ns %d" % (e, ns) for ns in (16, 32)
            for e in ("two blocks", "crossing", "crossing at two offsets", "short last range")})


# ------------------------------------------------------------------ inputs
def later_copies(groups, ns):
    """(groups, ns) bool: the columns that are exact copies of an EARLIER column of their own group"""
    dup = torch.zeros(groups, ns, dtype=torch.bool)
    for cls, (_, later) in enumerate(tie_pairs(ns)):
        dup[cls::4, later] = True
    return dup


def make_inputs(b, groups, ns, seed=0, device="cpu"):
    """Built directly on the CPU from a seeded generator and moved to `device`.
    y2 (b,128,groups,ns) = randn * 1.3 + 0.2; groups j with j % 4 == c carry pair c of tie_pairs(ns): the
    later column an exact copy of the kept one in all 128 channels, so every output channel ties.
    (scale, shift) of the input layer: float64 BatchNorm of y2 (gamma2 in +-[0.5, 1.5), every fifth negative,
    beta2 randn * 0.3) rounded to fp32; BIG_IN_CH: shift +30, scale +-0.05; SHUT_IN_CH: shift -50.
    w3 = randn / sqrt(128), row ZERO_ROW all zero, OFFSET_ROWS with 1.0 on a +30 input channel.
    gamma3 in +-[0.5, 1.5), every fifth negative, 0.0 at GAMMA3_ZERO_CH and -0.0 at GAMMA3_NEGZERO_CH;
    beta3 randn * 0.3."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * b + 10 * groups + ns)
    y2 = torch.randn(b, K_IN, groups, ns, generator=g) * 1.3 + 0.2
    for cls, (kept, later) in enumerate(tie_pairs(ns)):
        y2[:, :, cls::4, later] = y2[:, :, cls::4, kept]
    gamma2 = torch.rand(K_IN, generator=g) + 0.5
    gamma2[::5] *= -1
    beta2 = torch.randn(K_IN, generator=g) * 0.3
    yd = y2.double()
    mean = yd.mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(yd.var(dim=(0, 2, 3), unbiased=False) + EPS)
    del yd
    scale = (gamma2.double() * invstd).float()
    shift = (beta2.double() - mean * scale.double()).float()
    scale[BIG_IN_CH[0]], scale[BIG_IN_CH[1]] = BIG_SCALE, -BIG_SCALE
    shift[list(BIG_IN_CH)] = BIG_SHIFT
    shift[SHUT_IN_CH] = SHUT_SHIFT
    w3 = torch.randn(M_OUT, K_IN, generator=g) / K_IN ** 0.5
    w3[ZERO_ROW] = 0.0
    for row, ch in OFFSET_ROWS:
        w3[row, ch] = 1.0
    gamma3 = torch.rand(M_OUT, generator=g) + 0.5
    gamma3[::5] *= -1
    gamma3[GAMMA3_ZERO_CH] = 0.0
    gamma3[GAMMA3_NEGZERO_CH] = -0.0
    beta3 = torch.randn(M_OUT, generator=g) * 0.3
    dev = torch.device(device)
    out = {"b": b, "groups": groups, "ns": ns, "r": groups * ns, "eps": EPS, "momentum": MOMENTUM}
    for name, t in (("y2", y2), ("scale", scale), ("shift", shift), ("w3", w3), ("gamma3", gamma3), ("beta3", beta3)):
        out[name] = t.float().contiguous().to(dev)
    return out


# ------------------------------------------------------------------ truth and yardstick
def _bc(v, dtype):
    return v.to(dtype).view(1, -1, 1, 1)


def tile_pairs(y):
    """y (b,256,groups,ns) of any dtype -> (b * r / 64, 256, 2): (mean, M2) of every 64-column tile, two-pass,
    in y's dtype, in the order the kernels store them"""
    b, c = y.shape[0], y.shape[1]
    t = y.reshape(b, c, -1, TILE)
    mean = t.mean(3)
    m2 = ((t - mean.unsqueeze(3)) ** 2).sum(3)
    return torch.stack([mean, m2], dim=3).permute(0, 2, 1, 3).reshape(-1, c, 2).contiguous()


def _plant(y3, ns):
    """the copied columns' outputs are the same number (a library may sum two columns in different orders)"""
    for cls, (kept, later) in enumerate(tie_pairs(ns)):
        y3[:, :, cls::4, later] = y3[:, :, cls::4, kept]
    return y3


def _forward(inp, dtype):
    a2 = torch.relu(inp["y2"].to(dtype) * _bc(inp["scale"], dtype) + _bc(inp["shift"], dtype))
    y3 = torch.einsum("oc,bcmn->bomn", inp["w3"].to(dtype), a2)
    del a2
    if dtype == torch.float64:
        _plant(y3, inp["ns"])
    return _summary(y3, inp)


def _summary(y3, inp):
    """y3 (b,256,groups,ns) -> dict(y3, pairs, stats (as stats_of), win (value), idx (first index))"""
    v, idx = first_winner(y3, inp["gamma3"])
    win = v * pool_sign(inp["gamma3"]).to(y3.dtype).view(1, -1, 1)
    return {"y3": y3, "pairs": tile_pairs(y3), "win": win, "idx": idx,
            "stats": stats_of(y3, inp["gamma3"], inp["beta3"], inp["eps"], y3.dtype)}


def truth64(inp):
    return _forward(inp, torch.float64)


def plain_fp32(inp):
    with _tf32_off():
        return _forward(inp, torch.float32)


def split_form64(inp, products=SIX):
    """y3 as the kernel evaluates it, in float64: a2 = the fused multiply-add's one rounding to fp32, then the
    sum of the listed partial products (weight term, activation term) of the operands' bf16 terms, on the
    device of the inputs.  -> y3 (b,256,groups,ns) float64 (the accumulator's roundings are not modelled)"""
    dev = inp["y2"].device
    a2 = torch.relu(inp["y2"].double() * _bc(inp["scale"], torch.float64) + _bc(inp["shift"], torch.float64)).float()
    wt, at = bf16_terms(inp["w3"]), bf16_terms(a2)
    del a2
    y = 0
    for i in range(3):
        js = [j for (i2, j) in products if i2 == i]
        if js:
            y = y + torch.einsum("oc,bcmn->bomn", wt[i].to(dev), sum(at[j] for j in js).to(dev))
    return y


# ------------------------------------------------------------------ the conditions on the data
def check_inputs(inp, tru):
    """On the float64 truth, before anything is compared -> dict(offset: |mean| / std of OFFSET_ROWS, near:
    (b,256,groups) bool of the groups whose winner is within WIN_ULPS * ULP * range of its best rival that is
    not a copy, share: their share among the channels that are not constant, gate_slack).
    * every row of OFFSET_ROWS has |mean| / std >= MIN_OFFSET_RATIO, the constant channel variance exactly 0;
    * no ReLU gate of the input layer within GATE_ULPS fp32 roundings of zero;
    * SHUT_IN_CH is shut in every column, the +30 channels open in every column;
    * the copies are copies, in y2 and in the truth's y3;
    * share <= MAX_EXCLUDED (a seed that exceeds it is replaced)."""
    groups, ns = inp["groups"], inp["ns"]
    y2 = inp["y2"].double()
    prod = y2 * _bc(inp["scale"], torch.float64)
    z = prod + _bc(inp["shift"], torch.float64)
    slack = (z.abs() - GATE_ULPS * 2.0 ** -24 * (prod.abs() + _bc(inp["shift"], torch.float64).abs())).min().item()
    assert slack > 0, "a ReLU gate of the input layer within %d roundings of zero: take another seed" % GATE_ULPS
    assert bool((z[:, SHUT_IN_CH] < 0).all()) and bool((z[:, list(BIG_IN_CH)] > 20).all())
    del prod, z, y2
    st = tru["stats"]
    assert float(st["var"][ZERO_ROW]) == 0.0 and float(st["mean"][ZERO_ROW]) == 0.0
    live = torch.ones(M_OUT, dtype=torch.bool, device=st["var"].device)
    live[ZERO_ROW] = False
    assert bool((st["var"][live] > 0).all())
    rows = [row for row, _ in OFFSET_ROWS]
    ratio = st["mean"][rows].abs() / st["var"][rows].sqrt()
    assert len(rows) >= 3 and float(ratio.min()) >= MIN_OFFSET_RATIO, ratio.tolist()
    y3 = tru["y3"]
    for cls, (kept, later) in enumerate(tie_pairs(ns)):
        assert torch.equal(inp["y2"][:, :, cls::4, later], inp["y2"][:, :, cls::4, kept])
        assert torch.equal(y3[:, :, cls::4, later], y3[:, :, cls::4, kept])
    v = y3 * pool_sign(inp["gamma3"]).double().view(1, -1, 1, 1)
    v = torch.where(later_copies(groups, ns).to(v.device).view(1, 1, groups, ns), torch.full_like(v, -float("inf")), v)
    top = v.topk(2, dim=3)[0]
    del v
    rng = y3.abs().amax(dim=(0, 2, 3)).view(1, -1, 1)
    near = (top[..., 0] - top[..., 1]) <= WIN_ULPS * ULP * rng
    assert bool(near[:, ZERO_ROW].all())
    share = near[:, live].double().mean().item()
    assert share <= MAX_EXCLUDED, share
    return {"offset": ratio.tolist(), "near": near, "share": share, "gate_slack": slack}


# ------------------------------------------------------------------ the per-tile pairs: measures and floors
def _per_channel(d, scale):
    """d (tiles, c) >= 0, scale (c) -> (c): max over the tiles of d / scale; where scale = 0 the entry is 0 if d
    is 0 in every tile and inf if not"""
    worst = d.amax(0)
    return torch.where(scale > 0, worst / scale.clamp_min(1e-300),
                       torch.where(worst == 0, torch.zeros_like(worst), torch.full_like(worst, float("inf"))))


def pair_errors(got, want, var):
    """got, want (tiles,256,2), var (256) the float64 batch variance of the channels -> (mean: max over the
    tiles of |mean - mu_t| / sigma_c, m2: max over the tiles of |M2 - M2_t| / (64 var_c)), (256) tensors"""
    d = (got.double() - want.double()).abs()
    return _per_channel(d[:, :, 0], var.double().sqrt()), _per_channel(d[:, :, 1], TILE * var.double())


def pair_floors(y3, var):
    """What ONE fp32 ulp on every element of y3 (the float64 truth) is worth in a tile's pair (as
    sa1_train_cases.stat_floors: the sums are sums over fp32 values, and the part of their error that has one
    sign goes into a sum whole), in the measures of pair_errors:
      mean  ULP max_t mean_n |y| / sigma_c
      m2    d M2 = 2 sum (y - mu_t) dy: 2 ULP max_t sum_n |y - mu_t| |y| / (64 var_c), and one ulp of M2 itself
    0 where sigma_c = 0: a constant channel is exact"""
    b, c = y3.shape[0], y3.shape[1]
    t = y3.reshape(b, c, -1, TILE)
    mu = t.mean(3, keepdim=True)
    a_mean = t.abs().mean(3).amax(dim=(0, 2))
    a_m2 = ((t - mu).abs() * t.abs()).sum(3).amax(dim=(0, 2))
    m2 = ((t - mu) ** 2).sum(3).amax(dim=(0, 2))
    sig = var.double().sqrt()
    ok = sig > 0
    zero = torch.zeros_like(sig)
    return (torch.where(ok, ULP * a_mean / sig.clamp_min(1e-300), zero),
            torch.where(ok, ULP * (2 * a_m2 + m2) / (TILE * var.double()).clamp_min(1e-300), zero))


def own_pair_floors(want, var):
    """The pairs against those of the kernel's OWN stored y (want: float64 pairs of that y): one ulp of each
    output, in the measures of pair_errors (in the spirit of sa1_train_cases.own_floors)"""
    sig = var.double().sqrt()
    ok = sig > 0
    zero = torch.zeros_like(sig)
    return (torch.where(ok, ULP * want[:, :, 0].abs().amax(0) / sig.clamp_min(1e-300), zero),
            torch.where(ok, ULP * want[:, :, 1].amax(0) / (TILE * var.double()).clamp_min(1e-300), zero))


ONE_PASS_ROUNDINGS = {"t": 18, "tiled": 33}


def one_pass_floor(y3, var, layout):
    """The M2 of a tile as BOTH kernels form it: per half of a tile's 64 samples s2 - s1 * s1 / 32 from the
    sums s1 = sum d, s2 = sum d * d of d = y - c, shifted by the half's first sample c; the halves are merged
    with 16 dlt^2.  Two-pass fp32, the yardstick, subtracts the mean itself: it has no such terms, and one
    ulp of M2 does not cover them -- with c a few sigma off the half's mean, s2 and s1 * s1 / 32 are several
    times the difference they leave (measured on the device with that floor alone: need up to 4.8).
    The floor is the first-order bound of the roundings of these sums in fp32, u = ULP / 2 each, from the
    float64 truth y3 (b,256,groups,ns): a recursive sum of n roundings errs by at most n u times the sum of its
    terms' magnitudes (S2 for s2, A1 = sum |d| for s1), so per half
        |d M2_h| <= u (n S2 + 2 n A1 |S1| / 32 + 3 (S2 + S1^2 / 32))
    (the last term: the product, the division and the difference), n = ONE_PASS_ROUNDINGS[layout]:
      "t"      pool_fwd256_kernel: a half is the samples k of either chunk with (k >> 2) & 1 == h, its shift
               sample 4 h of the tile; packed sums of 16 terms, one addition of the two, one rounding of d
      "tiled"  gemm_nn2_kernel's row scan: the samples 32 h .. 32 h + 31, shift sample 32 h; 32 terms in turn
    -> (256) in pair_errors' measure of M2 (the worst tile of the channel); 0 where sigma_c = 0."""
    b, c = y3.shape[0], y3.shape[1]
    t = y3.reshape(b, c, -1, TILE)
    cols = torch.arange(TILE, device=y3.device)
    n = ONE_PASS_ROUNDINGS[layout]
    bound = 0
    for h in (0, 1):
        mine, first = (((cols >> 2) & 1) == h, 4 * h) if layout == "t" else ((cols >> 5) == h, 32 * h)
        d = t[..., mine] - t[..., first:first + 1]
        s2, s1, a1 = (d * d).sum(3), d.sum(3), d.abs().sum(3)
        bound = bound + n * s2 + 2 * n * a1 * s1.abs() / 32 + 3 * (s2 + s1 * s1 / 32)
    sig = var.double().sqrt()
    return torch.where(sig > 0, 0.5 * ULP * bound.amax(dim=(0, 2)) / (TILE * var.double()).clamp_min(1e-300),
                       torch.zeros_like(sig))


def finalize_fp32(pairs, n_part, gamma, beta, eps):
    """sa1_train_cases.finalize64's formula in plain fp32 torch ops: the yardstick of the finalize kernel"""
    p = pairs.float()
    n = float(p.shape[0]) * float(n_part)
    mean = p[:, :, 0].mean(0)
    m2 = p[:, :, 1].sum(0) + n_part * ((p[:, :, 0] - mean.view(1, -1)) ** 2).sum(0)
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    return mean, invstd, scale, beta - mean * scale
