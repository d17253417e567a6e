"""Shapes, index patterns, run census, inputs, float64 truth and fp32 yardstick for the tests of the first
shared-MLP layer applied BEFORE the gather (csrc/mlp_pregather.hip: pregather_pack_kernel,
pregather_unpack_kernel, pregather_forward_kernel, pregather_backward_kernel<4 | 8 | 16 | 32>); no package
import, everything here runs on the CPU.

The backward reads the m * ns entries of a cloud sorted by the point they refer to (group_inverse_kernel of
csrc/pn2_ball_group.hip).  Lane t of its 1024 owns the CHUNK consecutive sorted entries t * CHUNK ..
t * CHUNK + CHUNK - 1; CHUNK = 4 / 8 / 16 / 32 is the smallest with CHUNK * 1024 >= m * ns, the slots past
m * ns are pad (key 0xFFFF, after every point).  A RUN is the sorted entries of one point.  A run may lie
inside one lane, cross into the next or cover many lanes; the kernel stitches the pieces through four tables
in LDS, without atomics.

  SHAPES                        (case, b, c, n, m, ns), each inside the gate
  gate / chunk / forward_workgroups   the kernels' formulas restated; OUTSIDE: shapes just outside the gate
  PATTERNS, pattern_ok, index_rows, make_idx   the index arrays: one pattern per cloud, as many arrays per
                                shape as it takes to give every applicable pattern a cloud
  census(idx, n)                the classes (a) .. (i) of runs one cloud holds
  make_pack_inputs / pack_truth, unpack_truth
  make_forward_inputs / forward_truth / pair_truth64 / pair_plain_fp32 / pair_errors / pair_floors / pair_rule
  batch_stats64                 the layer's BatchNorm over all clouds, for the finalised coefficients
  make_exact_backward / exact_backward_truth      integer data: every sum is exact in fp32
  make_general_backward / general_backward_truth64 / general_backward_plain_fp32 / backward_errors
  kernel_form_pairs / kernel_form_backward        the kernels' own algebra in fp32 on the CPU
  check_inputs                  the conditions on the data, asserted before anything is compared
  within                        the rule  e(kernel) <= RATIO * e(plain fp32) + floor
"""
import torch

from sa1_train_cases import RATIO, ULP, f32   # noqa: F401  (RATIO = 3; ULP = 2^-23: one fp32 ulp, relative)

THREADS = 1024                # lanes of a workgroup, forward and backward
MAX_POINTS = 4096             # source row staged in LDS
MAX_GROUPS = 4096             # centroid row staged in LDS
MAX_ENTRIES = 32768           # gradient row staged in LDS
CB = 4                        # channels per workgroup of the forward kernel
WAVE = 64
EPS = 1e-5
MOMENTUM = 0.1

# (case, b, c, n, m, ns): the smallest shapes at which each mechanism is exercised
SHAPES = (
    ("one_quad", 1, 4, 1, 1, 4),             # one point, one group, one index quad; 1023 pad lanes
    ("nine_wgs", 3, 12, 37, 5, 4),           # 9 forward workgroups: xcd_block_id with a remainder; almost all pad
    ("pad_mid_lane", 2, 8, 1000, 1251, 4),   # m ns = 5004, CHUNK 8: the pad begins inside a lane
    ("no_pad", 2, 8, 512, 256, 16),          # m ns = 4096 = CHUNK 1024: lane 1023 is live (SA4's shape)
    ("sa3", 2, 8, 1024, 512, 16),            # CHUNK 8
    ("limits", 1, 4, 4096, 4096, 8),         # n, m, m ns at their limits, CHUNK 32, all eight index loads per lane
    ("wide_groups", 2, 4, 3, 100, 128),      # ns = 128, CHUNK 16, three points: every run covers hundreds of lanes
)
SHAPE_CHUNK = {"one_quad": 4, "nine_wgs": 4, "pad_mid_lane": 8, "no_pad": 4, "sa3": 8, "limits": 32, "wide_groups": 16}

# (what is off, b, c, n, m, ns): just outside the gate, one condition each
OUTSIDE = (
    ("c = 6", 1, 6, 64, 16, 4), ("ns = 2", 1, 4, 64, 16, 2), ("ns = 12", 1, 4, 64, 16, 12),
    ("n = 4097", 1, 4, 4097, 16, 4), ("m = 4097", 1, 4, 64, 4097, 4),
    ("m ns = 32768 + 4 ns", 1, 4, 64, 2052, 16),
)


def gate(b, c, n, m, ns):
    """pregather_shape_ok's formula (mlp_pregather_supported)"""
    return (b > 0 and 0 < c <= 65535 and c % CB == 0 and 0 < n <= MAX_POINTS and 0 < m <= MAX_GROUPS
            and ns >= 4 and ns & (ns - 1) == 0 and m * ns <= MAX_ENTRIES)


def chunk(mns):
    """inverse_chunk of csrc/pn2_ball_group.hip: sorted entries per lane"""
    c = 4
    while c * THREADS < mns:
        c *= 2
    return c


def forward_workgroups(b, c):
    return b * (c // CB)


def index_loads(mns):
    """(16-byte index loads a lane of the forward kernel issues at most, lanes that issue the last of them)"""
    n4 = mns // 4
    rounds = -(-n4 // THREADS)
    return rounds, n4 - (rounds - 1) * THREADS


# ------------------------------------------------------------------ index patterns
PATTERNS = ("ball", "one_point", "two_alternating", "each_once", "lane_runs", "lane_runs_shifted")


def pattern_ok(name, n, m, ns):
    mns = m * ns
    lanes = -(-mns // chunk(mns))               # live lanes = points lane_runs refers to
    if name == "two_alternating":
        return n >= 2
    if name == "each_once":
        return mns <= n
    if name == "lane_runs":
        return lanes <= n
    if name == "lane_runs_shifted":
        return lanes <= n and n >= 2 and mns >= 2
    return name in PATTERNS


def run_lengths(name, n, mns):
    """lane_runs: every referenced point exactly CHUNK times (the last one takes what is left of m ns).
    lane_runs_shifted: the lowest referenced point once, then the same -- every run straddles two lanes; where
    that would take one point more than the cloud has, the last point takes the rest (up to 2 CHUNK - 1)."""
    ch = chunk(mns)
    lens = [1] if name == "lane_runs_shifted" else []
    left = mns - sum(lens)
    while left > 0:
        take = left if len(lens) == n - 1 else min(ch, left)
        lens.append(take)
        left -= take
    return lens


def make_cloud_idx(name, n, m, ns, g):
    """one cloud's (m, ns) int64 index array, every value in [0, n)"""
    mns = m * ns
    if name == "ball":
        # random over the first three quarters of the points, two hot points, ball query's pads (the first
        # member repeated over the second half of the group)
        hi = max(1, (3 * n) // 4)
        idx = torch.randint(0, hi, (m, ns), generator=g)
        u = torch.rand(m, ns, generator=g)
        idx[u < 0.15] = hi // 3
        idx[u > 0.85] = (2 * hi) // 3
        idx[:, ns // 2:] = idx[:, :1]
        return idx
    if name == "one_point":
        return torch.full((m, ns), n - 1, dtype=torch.int64)
    if name == "two_alternating":
        flat = torch.empty(mns, dtype=torch.int64)
        flat[0::2] = (n - 1) // 2
        flat[1::2] = n - 1
        return flat.view(m, ns)
    if name == "each_once":
        return torch.randperm(n, generator=g)[:mns].view(m, ns)
    lens = run_lengths(name, n, mns)
    lo = 1 if n - 1 >= len(lens) else 0         # leave point 0 out where the cloud has a point to spare
    pts = (torch.randperm(n - lo, generator=g)[:len(lens)] + lo).sort()[0]
    flat = torch.repeat_interleave(pts, torch.tensor(lens))
    if name == "lane_runs":                     # positions scattered; the shifted form keeps equal neighbours
        flat = flat[torch.randperm(mns, generator=g)]
    return flat.view(m, ns)


def index_rows():
    """-> list of (case, b, c, n, m, ns, patterns): patterns[i] is cloud i's; every applicable pattern of a
    shape gets a cloud in one of its rows"""
    rows = []
    for case, b, c, n, m, ns in SHAPES:
        pats = [p for p in PATTERNS if pattern_ok(p, n, m, ns)]
        for r in range(-(-len(pats) // b)):
            rows.append((case, b, c, n, m, ns, tuple(pats[(r * b + i) % len(pats)] for i in range(b))))
    return rows


INDEX_ROWS = tuple(index_rows())


def row_id(row):
    return "%s-%s" % (row[0], "+".join(row[6]))


def _gen(row, salt):
    case, b, c, n, m, ns, pats = row
    h = sum((i + 1) * PATTERNS.index(p) for i, p in enumerate(pats))
    return torch.Generator().manual_seed(1000003 * salt + 7919 * h + 131 * n + 17 * m + ns + b + c)


def make_idx(row):
    """(b, m, ns) int32"""
    case, b, c, n, m, ns, pats = row
    g = _gen(row, 1)
    return torch.stack([make_cloud_idx(p, n, m, ns, g) for p in pats]).to(torch.int32).contiguous()


# ------------------------------------------------------------------ the run census
CLASSES = ("a_inside_lane", "b_one_boundary", "c_middle_lane", "d_wave_boundary", "e_ends_with_lane",
           "f_pad_same_lane", "f_pad_next_lane", "f_no_pad", "g_one_run", "h_unreferenced", "h_point_0",
           "h_point_last", "i_lane_1023_live", "i_lane_1023_covered", "i_lane_1023_continued")


def census(idx, n):
    """idx: one cloud's index array (any shape) -> dict class -> count, from a stable sort of the keys and
    lane = s // CHUNK:
      a  runs inside one lane              b  runs crossing exactly one lane boundary
      c  runs with at least one fully covered middle lane
      d  runs crossing a wave boundary (lane 64 k - 1 -> 64 k)
      e  runs whose last entry is the last entry of a lane while the next lane starts another key
      f  the last live run followed by pad in the same lane / in the next lane / not at all
      g  one run over every live entry     h  unreferenced points, point 0 and point n - 1 among them
      i  lane 1023 live / fully covered by one key / continued from lane 1022"""
    flat = idx.reshape(-1).long()
    mns = flat.numel()
    ch = chunk(mns)
    keys = flat.sort(stable=True)[0]
    start = torch.ones(mns, dtype=torch.bool)
    start[1:] = keys[1:] != keys[:-1]
    s0 = start.nonzero().view(-1)
    s1 = torch.cat([s0[1:] - 1, torch.tensor([mns - 1])])
    l0, l1 = s0 // ch, s1 // ch
    counts = torch.bincount(flat, minlength=n)
    last = (THREADS - 1) * ch
    live = mns > last
    return {
        "a_inside_lane": int((l0 == l1).sum()), "b_one_boundary": int((l1 == l0 + 1).sum()),
        "c_middle_lane": int((l1 >= l0 + 2).sum()), "d_wave_boundary": int((l0 // WAVE != l1 // WAVE).sum()),
        "e_ends_with_lane": int(((s1 % ch == ch - 1) & (s1 + 1 < mns)).sum()),
        "f_pad_same_lane": int(mns % ch != 0), "f_pad_next_lane": int(mns % ch == 0 and mns < ch * THREADS),
        "f_no_pad": int(mns == ch * THREADS), "g_one_run": int(s0.numel() == 1),
        "h_unreferenced": int((counts == 0).sum()), "h_point_0": int(counts[0] == 0),
        "h_point_last": int(counts[n - 1] == 0), "i_lane_1023_live": int(live),
        "i_lane_1023_covered": int(mns == ch * THREADS and bool(keys[last] == keys[mns - 1])),
        "i_lane_1023_continued": int(live and bool(keys[last - 1] == keys[last])),
    }


# ------------------------------------------------------------------ pack / unpack
# (b, c, n, m) beside the table's: n + m and n on, one short of and one past a multiple of 256
PACK_SHAPES = ((1, 1, 255, 2), (2, 3, 256, 256), (1, 2, 257, 254), (3, 5, 300, 213), (1, 4, 1, 1))
PACK_SCALES = (1.0, 1.0 / 0.8)


def pack_shapes():
    return PACK_SHAPES + tuple((b, c, n, m) for _, b, c, n, m, _ in SHAPES)


def make_pack_inputs(b, c, n, m):
    g = torch.Generator().manual_seed(40009 * b + 211 * c + 13 * n + m)
    return (torch.rand(b, n, 3, generator=g) * 4 - 2, torch.rand(b, m, 3, generator=g) * 4 - 2,
            torch.randn(b, c, n, generator=g))


def pack_truth(xyz, new_xyz, features, s):
    """cat([xyz s | new_xyz s ; features | 0]) in fp32: one multiplication by s rounded to fp32 per element"""
    s32 = torch.tensor(s, dtype=torch.float32)
    top = torch.cat([xyz.transpose(1, 2) * s32, new_xyz.transpose(1, 2) * s32], dim=2)
    b, c, _ = features.shape
    return torch.cat([top, torch.cat([features, torch.zeros(b, c, new_xyz.shape[1])], dim=2)], dim=1).contiguous()


def unpack_truth(dsrc_ext, n):
    return dsrc_ext[:, 3:, :n].contiguous()


# ------------------------------------------------------------------ forward
KINDS = ("big_mean", "outlier_first", "constant", "tiny_noise", "big_negative_mean", "plain")
BIG_MEAN = 40.0               # in units of the row's sigma (1)
OUTLIER = 6.0
# tiny_noise: multiples of 2^-16 (two ulps of 100) on 100.  A cloud's mean leaves the kernel as an fp32 number,
# half an ulp of LARGE off at most (ULP LARGE / 2 = 6e-6); the BatchNorm over the clouds squares the differences
# of those means, so its variance is off by up to (ULP LARGE)^2 / 2 = 7e-11 = 7e-6 of eps -- inside the 1e-5 the
# statistics tests hold invstd to.  (At LARGE = 1000 the same term is 7e-4 of eps: the format of the pair, not
# the kernel, would decide the test.)
LARGE = 100.0
NOISE_STEP = 2.0 ** -16
MIN_OFFSET = 20.0             # |mean| / sigma a big_mean row has at least (where the row is not constant)
MIN_OUTLIER = 5.0             # |first - mean| / sigma an outlier row reaches in at least one cloud of the table


def kind_of(ch):
    return KINDS[min(ch, len(KINDS) - 1)]


def make_forward_inputs(row):
    """z (b, c, n + m) fp32, by the kind of its channel (kind_of):
      big_mean / big_negative_mean   points +-40 + randn, centroids randn 0.3
      outlier_first   randn, and +6 on the point the first entry of the cloud refers to
      constant        points 2.5 + cloud, centroids -0.75: y is the same number everywhere
      tiny_noise      points 100 + k 2^-16 with k in -4 .. 4, centroids 0
      plain           randn 1.7 + 0.4, centroids randn 0.3
    and gamma (every third negative), beta, running statistics from random values"""
    case, b, c, n, m, ns, pats = row
    g = _gen(row, 2)
    idx = make_idx(row)
    z = torch.empty(b, c, n + m)
    for ch in range(c):
        kind = kind_of(ch)
        pts, cen = torch.randn(b, n, generator=g), torch.randn(b, m, generator=g) * 0.3
        if kind == "big_mean":
            pts += BIG_MEAN
        elif kind == "big_negative_mean":
            pts -= BIG_MEAN
        elif kind == "outlier_first":
            pts[torch.arange(b), idx[:, 0, 0].long()] += OUTLIER
        elif kind == "constant":
            pts = (2.5 + torch.arange(b, dtype=torch.float32)).view(b, 1).expand(b, n)
            cen = torch.full((b, m), -0.75)
        elif kind == "tiny_noise":
            pts = LARGE + torch.randint(-4, 5, (b, n), generator=g).float() * NOISE_STEP
            cen = torch.zeros(b, m)
        elif kind == "plain":
            pts = pts * 1.7 + 0.4
        z[:, ch, :n], z[:, ch, n:] = pts, cen
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::3] *= -1
    return {"row": row, "idx": idx, "z": z.contiguous(), "gamma": gamma, "beta": torch.randn(c, generator=g) * 0.3,
            "rm": torch.randn(c, generator=g) * 0.1, "rv": torch.rand(c, generator=g) + 0.5,
            "momentum": f32(MOMENTUM), "eps": f32(EPS)}


def forward_truth(z, idx, n):
    """y (b, c, m, ns) = z[:, :, idx] - z[:, :, n + j] in fp32: one subtraction per element"""
    b, c, w = z.shape
    m, ns = idx.shape[1], idx.shape[2]
    gathered = torch.gather(z, 2, idx.long().view(b, 1, m * ns).expand(b, c, m * ns)).view(b, c, m, ns)
    return gathered - z[:, :, n:].unsqueeze(-1)


def pair_truth64(y):
    """y (b, c, m, ns) fp32 -> (mean, M2, shift) (b, c) float64; shift = the row's first element"""
    r = y.double().flatten(2)
    mean = r.mean(2)
    return mean, ((r - mean.unsqueeze(-1)) ** 2).sum(2), r[:, :, 0]


def pair_plain_fp32(y):
    r = y.flatten(2)
    mean = r.mean(2)
    return mean, ((r - mean.unsqueeze(-1)) ** 2).sum(2)


def kernel_form_pairs(y):
    """pregather_forward_kernel's algebra in fp32 torch: sums of (y - shift) and its square about the row's
    first element, mean = shift + s1 / n, M2 = s2 - s1^2 / n (torch's order of summation, not the kernel's)"""
    r = y.flatten(2)
    n = torch.tensor(float(r.shape[2]))
    sh = r[:, :, :1]
    d = r - sh
    s1, s2 = d.sum(2), (d * d).sum(2)
    return sh.squeeze(2) + s1 / n, s2 - s1 * s1 / n


def pair_errors(got, tru, count):
    """got = (mean, M2) (b, c), tru = pair_truth64, count = m ns -> (|mean - mu| / sigma, |M2 - M2_t| / M2_t)
    as (b, c) float64; a constant row (M2_t = 0): 0 where the value is exact, inf where not"""
    mean, m2 = got[0].double(), got[1].double()
    mu, m2t, _ = tru
    sig = (m2t / float(count)).sqrt().clamp_min(1e-300)
    zero, inf = torch.zeros_like(mu), torch.full_like(mu, float("inf"))
    const = m2t == 0
    return (torch.where(const, torch.where(mean == mu, zero, inf), (mean - mu).abs() / sig),
            torch.where(const, torch.where(m2 == 0, zero, inf), (m2 - m2t).abs() / m2t.clamp_min(1e-300)))


# The longest chain of additions one term goes through in the forward kernel's sums: a lane adds up to eight
# rounds of ((d0 + d1) + (d2 + d3)) into its accumulator (2 + 8), the wave's butterfly has 6 steps, lane 0
# adds the 16 wave sums in turn.
PAIR_DEPTH = 2 + 8 + 6 + 16


def pair_floors(tru, count):
    """What the kernel's shifted-sum form can lose to rounding alone, worst case and to first order in ULP / 2
    per rounding.  With d_i = fl(y_i - shift) (one rounding), Delta = shift - mean, s1 = sum d_i = -n Delta,
    s2 = sum d_i^2 = M2 + n Delta^2 and D = PAIR_DEPTH roundings on the longest path of a sum:
      |err s1| <= (D + 1) ULP/2 sum |d_i|,  sum |d_i| <= sqrt(n s2)               (Cauchy-Schwarz)
      |err s2| <= (D/2 + 3/2) ULP s2                                               (d_i^2: 3 roundings)
      mean = shift + s1 / n:   |err| <= ULP ((D + 1)/2 sqrt(sigma^2 + Delta^2) + |Delta| / 2 + |mean| / 2)
      M2 = s2 - s1^2 / n:      |err s1^2 / n| <= 2 |s1| |err s1| / n + ULP n Delta^2
                                              <= (D + 1)/2 ULP (s2 + n Delta^2) + ULP n Delta^2     (AM-GM)
                               |err| <= ULP ((D + 5/2) M2 + (3 D / 2 + 7/2) n Delta^2)
    so the floor is proportional to ULP (M2 + n (shift - mean)^2).  -> (mean's floor in units of sigma, M2's
    relative floor), (b, c) float64; 0 on a constant row (every d_i is 0: both are exact)."""
    mu, m2, sh = tru
    n = float(count)
    sig = (m2 / n).sqrt()
    delta = (sh - mu).abs()
    d = float(PAIR_DEPTH)
    f_mean = ULP * ((d + 1) / 2 * (sig ** 2 + delta ** 2).sqrt() + delta / 2 + mu.abs() / 2)
    f_m2 = ULP * ((d + 2.5) * m2 + (1.5 * d + 3.5) * n * delta ** 2)
    const = m2 == 0
    zero = torch.zeros_like(mu)
    return (torch.where(const, zero, f_mean / sig.clamp_min(1e-300)),
            torch.where(const, zero, f_m2 / m2.clamp_min(1e-300)))


def pair_rule(got, y, tru=None):
    """got = (mean, M2) of y's rows under the rule against float64 -> [(name, ok, need, e, e32)] for the mean and
    for M2, the tiny-noise channel apart from the others (fp32 resolves its mean to a tenth of its sigma: its
    figures would hide every other row's).  On a constant row the yardstick counts as 0 (plain fp32's mean of
    4096 equal numbers is not that number): there the mean must be exact and M2 exactly 0."""
    count = y.shape[2] * y.shape[3]
    tru = pair_truth64(y) if tru is None else tru
    const = tru[1] == 0
    e = pair_errors(got, tru, count)
    e32 = [torch.where(const, torch.zeros_like(p), p) for p in pair_errors(pair_plain_fp32(y), tru, count)]
    floors = pair_floors(tru, count)
    tiny = [ch for ch in range(y.shape[1]) if kind_of(ch) == "tiny_noise"]
    rest = [ch for ch in range(y.shape[1]) if kind_of(ch) != "tiny_noise"]
    return [("%s, %s" % (name, tag),) + within(e[i][:, chs], e32[i][:, chs], floors[i][:, chs])
            for i, name in enumerate(("mean", "M2")) for tag, chs in (("tiny-noise row", tiny), ("other rows", rest))]


def batch_stats64(y, inp):
    """the layer's training-mode BatchNorm over all clouds in float64 -> dict(mean, var, invstd, scale, shift,
    running_mean, running_var)"""
    r = y.double().transpose(0, 1).flatten(1)
    n = r.shape[1]
    mean, var = r.mean(1), r.var(1, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + inp["eps"])
    scale = inp["gamma"].double() * invstd
    mom = inp["momentum"]
    return {"mean": mean, "var": var, "invstd": invstd, "scale": scale, "shift": inp["beta"].double() - mean * scale,
            "running_mean": (1 - mom) * inp["rm"].double() + mom * mean,
            "running_var": (1 - mom) * inp["rv"].double() + mom * var * (n / max(n - 1.0, 1.0)), "absmax": r.abs().max()}


# ------------------------------------------------------------------ backward
MAX_DZ = 8


def make_exact_backward(row):
    """scale 1, shift 0, coef (1, 0, 0), integer dz in [-8, 8]: transform<OP_DY> returns dz where y > 0 and 0
    elsewhere, every sum is an integer below 2^24.  y randn with exact zeros (+0 and -0: gate closed)."""
    case, b, c, n, m, ns, pats = row
    g = _gen(row, 3)
    y = torch.randn(b, c, m, ns, generator=g)
    u = torch.rand(b, c, m, ns, generator=g)
    y[u < 0.05] = 0.0
    y[u > 0.97] = -0.0
    dz = torch.randint(-MAX_DZ, MAX_DZ + 1, (b, c, m, ns), generator=g).float()
    one, zero = torch.ones(c), torch.zeros(c)
    coef = torch.stack([one, zero, zero], dim=1).contiguous()
    assert MAX_DZ * m * ns < 2 ** 24
    return {"row": row, "idx": make_idx(row), "y": y, "dz": dz, "scale": one, "shift": zero, "mean": zero.clone(),
            "invstd": one.clone(), "coef": coef}


def _scatter(values, idx, n):
    """values (b, c, m, ns), idx (b, m, ns) -> (b, c, n + m): sums over the entries of each point, then MINUS
    the sum of each group; in the dtype of values (CPU scatter_add_: the entries in index order)"""
    b, c, m, ns = values.shape
    out = torch.zeros(b, c, n + m, dtype=values.dtype)
    out[:, :, :n].scatter_add_(2, idx.long().view(b, 1, m * ns).expand(b, c, m * ns), values.reshape(b, c, m * ns))
    out[:, :, n:] = -values.sum(3)
    return out


def exact_backward_truth(inp):
    """int64 scatter-add of the gated dz over idx, minus the group sums -> (b, c, n + m) int64"""
    n = inp["row"][3]
    gated = torch.where(inp["y"] > 0, inp["dz"], torch.zeros(())).long()
    return _scatter(gated, inp["idx"], n)


BIG_MU = 40.0                 # rows with |mu| = 40 / invstd: channels 1, 5, 9, ...


def make_general_backward(row):
    """invstd in [0.5, 1.5), mu randn (+-40 / invstd on channels 1 mod 4), gamma +-[0.5, 1.5) with every third
    negative, beta randn 0.3, scale = gamma invstd, shift = beta - mu scale (fp32), coef = (scale, c1, c2) with
    c1, c2 randn 0.1 (c1 signed against invstd c2 mu), y = mu + randn / invstd, dz randn"""
    case, b, c, n, m, ns, pats = row
    g = _gen(row, 4)
    invstd = torch.rand(c, generator=g) + 0.5
    mu = torch.randn(c, generator=g)
    sign = torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    mu[1::4] = (sign * BIG_MU / invstd)[1::4]
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::3] *= -1
    beta = torch.randn(c, generator=g) * 0.3
    scale = gamma * invstd
    shift = beta - mu * scale
    c1, c2 = torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1
    # c1 takes the sign that does not cancel against invstd c2 mu: P = |p| below, and the floor is at most 3 ULP
    # of the mass (with cancellation it grows by P / |p|, which is a property of the data, not of the kernel)
    c1 = torch.where(invstd * c2 * mu > 0, -c1.abs(), c1.abs())
    coef = torch.stack([scale, c1, c2], dim=1)
    y = mu.view(1, c, 1, 1) + torch.randn(b, c, m, ns, generator=g) / invstd.view(1, c, 1, 1)
    return {"row": row, "idx": make_idx(row), "y": y.contiguous(), "dz": torch.randn(b, c, m, ns, generator=g),
            "scale": scale, "shift": shift, "mean": mu, "invstd": invstd, "coef": coef.contiguous()}


def _col(v, dtype):
    return v.to(dtype).view(1, -1, 1, 1)


def open_gate(inp):
    """(y scale + shift > 0) in float64 from the promoted operands: the product of two fp32 numbers is exact in
    float64 and the sum's sign is the exact sum's, which is the sign of the fused multiply-add's result"""
    return inp["y"].double() * _col(inp["scale"], torch.float64) + _col(inp["shift"], torch.float64) > 0


def general_backward_truth64(inp):
    """-> (truth (b, c, n + m), mass, floor_abs): float64.
    truth: scatter of the unfolded a (g - c1 - (y - mu) is c2) from the fp32 coefficients.
    mass = sum over the run of |a g| + |q y| + |p| with q = -a is c2, p = a (is c2 mu - c1) as load_row_coef
    folds them.
    floor_abs: what the fold and the two fused multiply-adds lose to rounding alone, summed over the run, to
    first order with ULP / 2 per rounding: q = -fl(a fl(is c2)) has two (|err q| <= ULP |q|); p =
    fl(a fl(fl(fl(is c2) mu) - c1)) has four, each at most ULP / 2 of P = |a| (|is c2 mu| + |c1|) >= |p|
    (|err p| <= 2 ULP P); lin = fma(q, y, p) one, ULP / 2 (|q y| + |p|); fma(a, dz, lin) one, ULP / 2 (|a g| +
    |q y| + |p|):   |err| <= ULP (|a g| / 2 + 2 |q y| + |p| + 2 P),  at most 3 ULP of the mass where P = |p|."""
    d = torch.float64
    n = inp["row"][3]
    y, coef = inp["y"].double(), inp["coef"].double()
    a, c1, c2 = (_col(coef[:, i].contiguous(), d) for i in range(3))
    mu, inv = _col(inp["mean"], d), _col(inp["invstd"], d)
    g = torch.where(open_gate(inp), inp["dz"].double(), torch.zeros((), dtype=d))
    dy = a * (g - c1 - (y - mu) * inv * c2)
    q, p = -a * inv * c2, a * (inv * c2 * mu - c1)
    big_p = a.abs() * ((inv * c2 * mu).abs() + c1.abs())
    ag, qy = (a * g).abs(), (q * y).abs()
    mass = ag + qy + p.abs()
    floor_abs = ULP * (ag / 2 + 2 * qy + p.abs() + 2 * big_p)
    idx = inp["idx"]
    # (the group sums' sign plays no part in a mass)
    return _scatter(dy, idx, n), _scatter(mass, idx, n).abs(), _scatter(floor_abs.expand_as(mass), idx, n).abs()


def general_backward_plain_fp32(inp):
    """the yardstick: the unfolded formula in fp32 torch ops behind the truth's gate, summed by fp32
    scatter_add_ / sum"""
    f = torch.float32
    n = inp["row"][3]
    coef = inp["coef"]
    a, c1, c2 = (_col(coef[:, i].contiguous(), f) for i in range(3))
    g = torch.where(open_gate(inp), inp["dz"], torch.zeros(()))
    dy = a * (g - c1 - (inp["y"] - _col(inp["mean"], f)) * _col(inp["invstd"], f) * c2)
    return _scatter(dy, inp["idx"], n)


def _fma32(x, y, z):
    """fma of fp32 tensors through float64 (the product is exact there; the sum is rounded twice)"""
    return (x.double() * y.double() + z.double()).float()


def kernel_form_backward(inp, swap_c=False, sign=-1.0):
    """load_row_coef<OP_DY> and transform<OP_DY> of csrc/mlp_operand.h in fp32 on the CPU, summed by fp32
    scatter_add_ (not the kernel's order).  swap_c / sign: the mutants the CPU test fails the rule with."""
    n = inp["row"][3]
    coef = inp["coef"]
    a, c1, c2 = coef[:, 0], coef[:, 1 + int(swap_c)], coef[:, 2 - int(swap_c)]
    t = inp["invstd"] * c2
    q = -(a * t)
    p = a * (t * inp["mean"] - c1)
    f = torch.float32
    y = inp["y"]
    z = _fma32(y, _col(inp["scale"], f), _col(inp["shift"], f))
    lin = _fma32(_col(q, f).expand_as(y), y, _col(p, f))
    r = torch.where(z > 0, _fma32(_col(a, f).expand_as(y), inp["dz"], lin), lin)
    out = _scatter(r, inp["idx"], n)
    out[:, :, n:] *= -sign
    return out


def backward_errors(got, truth, mass):
    """|got - truth| / mass per element, float64; mass 0 (an unreferenced point): 0 where got is 0, inf where not"""
    d = (got.double() - truth).abs()
    dead = mass == 0
    return torch.where(dead, torch.where(got.double() == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))),
                       d / mass.clamp_min(1e-300))


def backward_floor(mass, floor_abs):
    return torch.where(mass == 0, torch.zeros_like(mass), floor_abs / mass.clamp_min(1e-300))


# ------------------------------------------------------------------ the conditions on the data, the rule
def check_inputs(row):
    """On one index row, before anything is compared -> dict of figures.
    * idx lies in [0, n); the gate formula holds; CHUNK is the table's;
    * forward: the constant row is constant in fp32 (float64 M2 exactly 0) and no other row is; the big-mean
      rows have |mean| / sigma >= MIN_OFFSET wherever the cloud's row is not constant; the tiny-noise row is
      100 + k 2^-16, |k| <= 4; the outlier figure |first - mean| / sigma is returned per cloud;
    * exact backward: dz integer, |dz| <= 8, both states of the gate and exact zeros of y present (where the
      tensor has more than a handful of elements);
    * general backward: both states of the gate present, some rows with |mu| invstd = 40, no gate value at 0."""
    case, b, c, n, m, ns, pats = row
    assert gate(b, c, n, m, ns) and chunk(m * ns) == SHAPE_CHUNK[case]
    idx = make_idx(row)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (b, m, ns)
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    info = {}
    fwd = make_forward_inputs(row)
    y = forward_truth(fwd["z"], idx, n)
    mean, m2, first = pair_truth64(y)
    sig = (m2 / (m * ns)).sqrt()
    outlier = []
    for ch in range(c):
        kind = kind_of(ch)
        for cl in range(b):
            const = float(m2[cl, ch]) == 0.0
            if kind == "constant":
                assert const and float(mean[cl, ch]) == 3.25 + cl
            elif kind in ("big_mean", "big_negative_mean") and not const:
                assert float(mean[cl, ch].abs() / sig[cl, ch]) >= MIN_OFFSET, (kind, cl, ch)
            elif kind == "tiny_noise":
                assert float((y[cl, ch].double() - LARGE).abs().max()) <= 4 * NOISE_STEP
            elif kind == "outlier_first" and not const:
                outlier.append(float((first[cl, ch] - mean[cl, ch]).abs() / sig[cl, ch]))
    info["outlier"] = max(outlier) if outlier else 0.0
    info["constant_rows"] = int((m2 == 0).sum())
    ex = make_exact_backward(row)
    assert torch.equal(ex["dz"], ex["dz"].round()) and float(ex["dz"].abs().max()) <= MAX_DZ
    if ex["y"].numel() >= 256:
        assert bool((ex["y"] > 0).any()) and bool((ex["y"] < 0).any()) and bool((ex["y"] == 0).any())
    gen = make_general_backward(row)
    zg = gen["y"].double() * _col(gen["scale"], torch.float64) + _col(gen["shift"], torch.float64)
    assert not bool((zg == 0).any())
    if gen["y"].numel() >= 256:
        share = float((zg > 0).double().mean())
        assert 0.1 < share < 0.9, share
    ratio = (gen["mean"].abs() * gen["invstd"])[1::4]
    assert bool(((ratio - BIG_MU).abs() < 1e-3).all())
    return info


def within(e, e32, floor, over=None):
    """The rule, element by element: e <= RATIO * yardstick + floor.  over = dims: the yardstick is plain
    fp32's WORST figure over those dims (the backward: over a cloud's channels and outputs, so that one lucky
    fp32 sum cannot fail a kernel sum, while a cloud of long runs does not loosen a cloud of short ones);
    over = None: plain fp32's figure of that very row (the pairs: the floors there bound the kernel's form
    by themselves, and plain fp32's mean of the tiny-noise row is off by a good part of its sigma).
    -> (ok, need = max e / bound, worst e, worst e32)"""
    yard = e32 if over is None else e32.amax(dim=over, keepdim=True)
    bound = RATIO * yard + floor
    exact = bound == 0
    need = torch.where(exact, torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))),
                       e / bound.clamp_min(1e-300))
    return bool((e <= bound).all()), float(need.max()), float(e.max()), float(e32.max())
