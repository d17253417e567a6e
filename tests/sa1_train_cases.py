"""Shapes, inputs, float64 truth and fp32 yardstick for the tests of set abstraction 1's TRAINING forward
(csrc/mlp_chain.hip: chain_prep_kernel, chain_lin4_kernel<4, NS, FULL> for NS = 16 / 32 / 64 as statistics
pass and full pass, chain_finalize_kernel; csrc/mlp_first4.hip: moments, BatchNorm from the moments, the
first layer's weight gradient from gated sums and the moments); no package import.

Layers are numbered as the kernels number them: layer 1 is the virtual 4 -> 64 layer (w0, coeff0), layer 2
the 64 -> 64 layer (w1, gamma1, beta1), layer 3 the 64 -> 128 layer behind the max-pool (w2, gamma2, beta2).

A tile is 32 consecutive columns of one cloud, a wave owns 2 consecutive tiles, a workgroup 4 waves: 8
tiles = 256 columns, and the gate r = m * ns % 256 == 0 makes every cloud a whole number of workgroups.
Each workgroup leaves one (mean, M2) pair per channel: parts = workgroups.

  CHAIN_SHAPES                  (case, ns, b, m, tiles_per_cloud, workgroups, seed, momentum, running)
  chain_arith / chain_gate      the formulas tests/test_sa1_train_cases.py checks the table with
  make_chain_inputs(b, m, ns, seed, momentum, running)   see its docstring
  truth64(inp)                  the reference module's layers in float64 from the fp32 operands promoted: conv
                                1x1 without bias, BatchNorm2d on batch statistics (biased variance, unbiased in
                                the running estimate), ReLU, max over nsample -- pytorch_utils.py:14-39,70-124,
                                pointnet2_modules.py:256-262 -- behind the given affine + ReLU of layer 1
  plain_fp32(inp)               the same in fp32 torch ops (einsum with TF32 off, mean, var): the yardstick
  check_inputs(inp, tru)        the conditions on the data, asserted before anything is compared
  tensor_errors / tensor_floors, stat_errors / stat_floors / own_floors, running_errors, within(...)
                                the measures, the floors the number format alone gives them, and the rule
                                e(kernel) <= RATIO * e(plain fp32) + floor
  split_form64(inp, products)   the two GEMMs in float64 from the operands' bf16 terms, keeping the listed
                                partial products (mlp_frag.h: mfma6 keeps SIX of the nine)
  finalize64(...)               chain_finalize_kernel's pooled-variance formula in float64
  FIRST4_SHAPES, first4_slices, make_first4_inputs, first4_truth64, first4_plain_fp32, check_first4_inputs
                                the first layer's weight gradient: inputs from float64 torch rounded to fp32
                                (no kernel of the project prepares them), truth = float64 autograd
  MOMENT_SHAPES, moments64, first4_bn_truth64, first4_bn_plain_fp32
"""
import contextlib

import torch

RATIO = 3                     # e(kernel) <= RATIO * e(plain fp32): eval_pool_cases.RATIO, pool_gram256_cases.RATIO
ULP = 2.0 ** -23              # one fp32 ulp of a value, relative to it, at most
EPS = 1e-5
BIG_MEAN = 40.0
BIG_CH_LIN4 = (3, 21, 40, 62)  # layer-1 channels with +30 in the shift: one per (k step, half-wave) corner
BIG_SHIFT = 30.0
BIG_BETA1_CH = (5, 30, 58)    # beta1 = +30: layer 3's input has channels with mean 30
ZERO_ROW1, ZERO_ROW2 = 17, 77  # all-zero rows of w1 / w2: that output channel is the constant 0
GAMMA2_ZERO_CH = 33           # gamma2 == 0.0 exactly
TIE_EVERY = 7                 # the groups 0, 7, 14, ... carry the copied columns
TIES = ((1, 3), (2, 5))       # (kept, later copy): within a half-wave; across the half-waves
TIE_64 = (6, 38)              # ns = 64: across the two tiles of a group
BORDER_MOD = (0, 8)           # ns = 16: groups j with j % 14 in BORDER_MOD (even: both groups in one tile)
                              # hand their sample 15 to sample 0 of group j + 1
MIN_OFFSET_RATIO = 20.0       # |mean| / std of the two most offset output channels of each layer, at least
WIN_ULPS = 4                  # a layer-3 winner is at least WIN_ULPS * ULP * range ahead of its rival
GATE_ULPS = 4                 # first4: |z| > GATE_ULPS * 2^-24 * (|scale| sum |w x| + |shift|)
MAX_EXCLUDED = 0.01

# (case, ns, b, m, tiles_per_cloud, workgroups, seed, momentum, running buffers given)
# The seeds are those at which check_inputs holds (tests/test_sa1_train_cases.py runs it on every row).
CHAIN_SHAPES = (
    ("one_wg", 16, 1, 16, 8, 1, 0, 0.1, True), ("one_wg", 32, 1, 8, 8, 1, 0, 0.1, True),
    ("one_wg", 64, 1, 4, 8, 1, 0, 0.1, True),
    ("one_wg_b3", 16, 3, 16, 8, 3, 0, 0.37, True), ("one_wg_b3", 32, 3, 8, 8, 3, 0, 0.37, True),
    ("one_wg_b3", 64, 3, 4, 8, 3, 0, 0.37, True),
    ("three_wg", 16, 2, 48, 24, 6, 0, 0.1, False), ("three_wg", 32, 2, 24, 24, 6, 0, 0.1, True),
    ("three_wg", 64, 2, 12, 24, 6, 0, 0.1, True),
    ("sevenths", 16, 2, 112, 56, 14, 0, 0.1, True), ("sevenths", 32, 2, 56, 56, 14, 0, 0.1, True),
    ("sevenths", 64, 2, 28, 56, 14, 0, 0.1, True),
)
COLS_PER_PART = 256


def chain_gate(b, m, ns):
    """chain_shape_ok's formula (mlp_chain_lin4_parts > 0)"""
    return b > 0 and m > 0 and ns in (16, 32, 64) and (m * ns) % 256 == 0


def chain_arith(b, m, ns):
    """-> (tiles_per_cloud, workgroups = parts); eval_pool_cases.tile_arith at two tiles per wave"""
    r = m * ns
    assert r % 32 == 0
    tpc = r // 32
    total = b * tpc
    assert total % 8 == 0
    return tpc, total // 8


@contextlib.contextmanager
def _tf32_off():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old


def f32(v):
    """a Python float rounded to fp32 (what crosses the C ABI as `float`)"""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------ the chain's inputs
def later_copies(m, ns):
    """(m, ns) bool: the columns that are exact copies of an EARLIER column of their own group"""
    dup = torch.zeros(m, ns, dtype=torch.bool)
    for _, later in TIES + ((TIE_64,) if ns == 64 else ()):
        dup[::TIE_EVERY, later] = True
    return dup


def border_groups(m, ns):
    """ns = 16: the groups j whose sample 15 is copied to sample 0 of group j + 1 (same tile, other group)"""
    if ns != 16:
        return []
    return [j for j in range(0, m - 1) if j % 14 in BORDER_MOD]


def plant_ties(x4):
    """exact copies of columns (all four channels), in place; x4 (b,4,m,ns)"""
    m, ns = x4.shape[2], x4.shape[3]
    for kept, later in TIES + ((TIE_64,) if ns == 64 else ()):
        x4[:, :, ::TIE_EVERY, later] = x4[:, :, ::TIE_EVERY, kept]
    for j in border_groups(m, ns):
        x4[:, :, j + 1, 0] = x4[:, :, j, 15]
    return x4


def make_chain_inputs(b, m, ns, seed=0, momentum=0.1, running=True, device="cpu"):
    """Built directly, as eval_pool_cases.weights does: what is measured is the kernels, not the BatchNorm
    fold in front of them.
    x4 (b,4,m,ns) randn, channel 3 at randn * 2 + 40, with the copied columns of plant_ties.
    w0 (64,4) with column 3 damped (x 0.05); coeff0 = (scale0, shift0): about 20 % of the scales negative,
    the shift cancels the mean of 40 (-40 scale0 w0[:, 3] + O(0.2)) and carries +30 on BIG_CH_LIN4.
    w1 (64,64), w2 (128,64), randn / 8, row ZERO_ROW1 / ZERO_ROW2 all zero.  gamma1 / gamma2 in
    +-[0.5, 1.5) with every fifth negative, gamma2[GAMMA2_ZERO_CH] = 0.0; beta randn * 0.3, beta1 = +30 on
    BIG_BETA1_CH.  Running statistics start from random values (mean randn * 0.1, variance in [0.5, 1.5));
    running=False passes none."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * b + 10 * m + ns)
    x4 = torch.randn(b, 4, m, ns, generator=g)
    x4[:, 3] = x4[:, 3] * 2 + BIG_MEAN
    plant_ties(x4)
    w0 = torch.randn(64, 4, generator=g) * 0.7
    w0[:, 3] *= 0.05
    sign = torch.where(torch.rand(64, generator=g) < 0.2, -1.0, 1.0)
    sc0 = sign * (0.5 + torch.rand(64, generator=g))
    sh0 = -BIG_MEAN * sc0 * w0[:, 3] + torch.randn(64, generator=g) * 0.2
    sh0[list(BIG_CH_LIN4)] += BIG_SHIFT
    w1 = torch.randn(64, 64, generator=g) / 8
    w2 = torch.randn(128, 64, generator=g) / 8
    w1[ZERO_ROW1] = 0.0
    w2[ZERO_ROW2] = 0.0

    def bn(c):
        gamma = torch.rand(c, generator=g) + 0.5
        gamma[::5] *= -1
        return gamma, torch.randn(c, generator=g) * 0.3, torch.randn(c, generator=g) * 0.1, \
            torch.rand(c, generator=g) + 0.5

    g1, be1, rm1, rv1 = bn(64)
    g2, be2, rm2, rv2 = bn(128)
    be1[list(BIG_BETA1_CH)] = BIG_SHIFT
    g2[GAMMA2_ZERO_CH] = 0.0
    dev = torch.device(device)
    out = {"b": b, "m": m, "ns": ns, "r": m * ns, "momentum": f32(momentum), "eps": f32(EPS), "running": running}
    for name, t in (("x4", x4), ("w0", w0), ("sc0", sc0), ("sh0", sh0), ("w1", w1), ("w2", w2), ("g1", g1),
                    ("be1", be1), ("rm1", rm1), ("rv1", rv1), ("g2", g2), ("be2", be2), ("rm2", rm2), ("rv2", rv2)):
        out[name] = t.float().contiguous().to(dev)
    return out


# ------------------------------------------------------------------ truth and yardstick
def _bc(v, dtype):
    return v.to(dtype).view(1, -1, 1, 1)


def _layers(inp, dtype):
    """-> dict: y2, y3 (raw outputs), per layer (mean, var (biased), invstd, scale, shift), the new running
    statistics, pooled (b,128,m) -- all in `dtype`, from torch ops on the fp32 operands cast to it"""
    n = inp["b"] * inp["r"]
    mom, eps = inp["momentum"], inp["eps"]
    y0 = torch.einsum("oc,bcmn->bomn", inp["w0"].to(dtype), inp["x4"].to(dtype))
    a = torch.relu(y0 * _bc(inp["sc0"], dtype) + _bc(inp["sh0"], dtype))
    out = {}
    for layer, (w, gamma, beta, rm, rv) in ((2, ("w1", "g1", "be1", "rm1", "rv1")), (3, ("w2", "g2", "be2", "rm2", "rv2"))):
        y = torch.einsum("oc,bcmn->bomn", inp[w].to(dtype), a)
        mean = y.mean(dim=(0, 2, 3))
        var = y.var(dim=(0, 2, 3), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + eps)
        scale = inp[gamma].to(dtype) * invstd
        shift = inp[beta].to(dtype) - mean * scale
        out["y%d" % layer] = y
        out["stats%d" % layer] = {"mean": mean, "var": var, "invstd": invstd, "scale": scale, "shift": shift}
        out["running%d" % layer] = ((1 - mom) * inp[rm].to(dtype) + mom * mean,
                                    (1 - mom) * inp[rv].to(dtype) + mom * (var * (n / (n - 1.0))))
        a = torch.relu(y * _bc(scale, dtype) + _bc(shift, dtype))
    out["pooled"] = a.amax(3)
    return out


def truth64(inp):
    return _layers(inp, torch.float64)


def plain_fp32(inp):
    with _tf32_off():
        return _layers(inp, torch.float32)


def pool_sign(gamma2):
    """which extreme of a channel wins the pool: -1 where gamma2 < 0, +1 elsewhere (relu(y scale + shift) is
    monotone in y; chain_lin4_kernel's `sgn`)"""
    return torch.where(gamma2 < 0, -1.0, 1.0).to(gamma2.dtype)


def first_winner(y3, gamma2):
    """y3 (b,128,m,ns) -> (value of sign * y at its maximum over the group, FIRST index attaining it); exact
    in the dtype of y3 (a multiplication by +-1)"""
    v = y3 * pool_sign(gamma2).to(y3.dtype).view(1, -1, 1, 1)
    mx = v.amax(3, keepdim=True)
    ns = y3.shape[3]
    pos = torch.arange(ns, device=y3.device).view(1, 1, 1, ns).expand_as(v)
    first = torch.where(v == mx, pos, torch.full_like(pos, ns)).amin(3)
    return mx.squeeze(3), first


# ------------------------------------------------------------------ the conditions on the data
def check_inputs(inp, tru):
    """On the float64 truth, before anything is compared -> dict(offset2, offset3: the two largest |mean| / std
    per layer, near: (b,128,m) bool of the layer-3 groups whose winner is within WIN_ULPS * ULP * range of its
    rival, share: their share among the channels that are not constant).
    * each layer has at least two output channels with |mean| / std >= MIN_OFFSET_RATIO;
    * the constant channels (the zero rows of w1 / w2) have variance exactly 0, every other channel does not;
    * the later copy of a tied pair never counts as a rival; apart from those, the share of groups whose
      winner is not clear of its rival is at most MAX_EXCLUDED (a seed that exceeds it is replaced)."""
    b, m, ns = inp["b"], inp["m"], inp["ns"]
    info = {}
    for layer, zero_row in ((2, ZERO_ROW1), (3, ZERO_ROW2)):
        st = tru["stats%d" % layer]
        assert float(st["var"][zero_row]) == 0.0 and float(st["mean"][zero_row]) == 0.0
        live = torch.ones_like(st["var"], dtype=torch.bool)
        live[zero_row] = False
        assert bool((st["var"][live] > 0).all())
        ratio = (st["mean"][live].abs() / st["var"][live].sqrt()).sort(descending=True)[0]
        assert float(ratio[1]) >= MIN_OFFSET_RATIO, (layer, ratio[:4].tolist())
        info["offset%d" % layer] = ratio[:2].tolist()
    y3 = tru["y3"]
    x4 = inp["x4"]
    for kept, later in TIES + ((TIE_64,) if ns == 64 else ()):   # the copies are copies
        assert torch.equal(x4[:, :, ::TIE_EVERY, later], x4[:, :, ::TIE_EVERY, kept])
        assert torch.equal(y3[:, :, ::TIE_EVERY, later], y3[:, :, ::TIE_EVERY, kept])
    for j in border_groups(m, ns):
        assert torch.equal(y3[:, :, j + 1, 0], y3[:, :, j, 15])
    v = y3 * pool_sign(inp["g2"]).double().view(1, -1, 1, 1)
    v = torch.where(later_copies(m, ns).to(v.device).view(1, 1, m, ns), torch.full_like(v, -float("inf")), v)
    top = v.topk(2, dim=3)[0]
    rng = y3.abs().amax(dim=(0, 2, 3)).view(1, -1, 1)
    near = (top[..., 0] - top[..., 1]) <= WIN_ULPS * ULP * rng
    live = torch.ones(128, dtype=torch.bool, device=near.device)
    live[ZERO_ROW2] = False
    assert bool(near[:, ZERO_ROW2].all())
    share = near[:, live].double().mean().item()
    assert share <= MAX_EXCLUDED, share
    info["near"], info["share"] = near, share
    return info


# ------------------------------------------------------------------ measures, floors, the rule
def _sigma(var):
    return var.double().sqrt()


def tensor_errors(v, t, var):
    """v, t (b,c,...) with the channel on axis 1, var (c) the float64 variance of t's channels ->
    (global: max |v - t| / max |t|, per channel: max_n |v - t|_c / sigma_c as a (c) tensor; where sigma_c = 0
    the entry is 0 if v equals t there exactly and inf if not)"""
    c = t.shape[1]
    d = (v.double() - t).abs().transpose(0, 1).reshape(c, -1).amax(1)
    sig = _sigma(var)
    per = torch.where(sig > 0, d / sig.clamp_min(1e-300),
                      torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    return (d.max() / t.abs().max()).item(), per


def tensor_floors(t, var):
    """What the fp32 format of the output resolves: one ulp of the range in the global measure, one ulp of the
    channel's range over sigma_c per channel (0 where sigma_c = 0: a constant channel is exact)"""
    c = t.shape[1]
    rng = t.abs().transpose(0, 1).reshape(c, -1).amax(1)
    sig = _sigma(var)
    return ULP, torch.where(sig > 0, ULP * rng / sig.clamp_min(1e-300), torch.zeros_like(sig))


def stat_errors(got, st):
    """got = (mean, invstd, scale, shift) of any dtype, st = the truth's dict, gamma inside st["gamma"] ->
    dict of (c) tensors:
      mean    |mean - mu_c| / sigma_c                (sigma_c = 0: |mean - mu_c| / |mu_c|, 0 where both are 0)
      invstd  |invstd sqrt(var_c + eps) - 1|
      scale   |scale - gamma invstd_c| / |gamma invstd_c|     (gamma = 0: 0 if scale is 0, inf if not)
      shift   |shift - shift_c| / |gamma|: the error it leaves in units of xhat   (gamma = 0: 0 / inf on equality)"""
    mean, invstd, scale, shift = (x.double() for x in got)
    sig, gamma = _sigma(st["var"]), st["gamma"].double()
    inf = torch.full_like(sig, float("inf"))
    zero = torch.zeros_like(sig)
    dm = (mean - st["mean"]).abs()
    e_mean = torch.where(sig > 0, dm / sig.clamp_min(1e-300),
                         torch.where(dm == 0, zero, dm / st["mean"].abs().clamp_min(1e-300)))
    e_inv = (invstd / st["invstd"] - 1).abs()
    live = gamma != 0
    e_scale = torch.where(live, (scale - st["scale"]).abs() / st["scale"].abs().clamp_min(1e-300),
                          torch.where(scale == 0, zero, inf))
    e_shift = torch.where(live, (shift - st["shift"]).abs() / gamma.abs().clamp_min(1e-300),
                          torch.where(shift == st["shift"], zero, inf))
    return {"mean": e_mean, "invstd": e_inv, "scale": e_scale, "shift": e_shift}


def stat_floors(t, st):
    """What ONE fp32 ulp on every element of the layer's output t is worth in its statistics (the sums are
    sums over fp32 values; a part of their error that has one sign goes into a sum whole -- DESIGN.md,
    Gram-256 section), per channel:
      mean    ULP mean_n |t_c| / sigma_c                      (sigma_c = 0: ULP, one ulp of the mean itself)
      invstd  ULP mean_n (|t_c - mu_c| |t_c|) / (var_c + eps): half the relative change of the variance
      scale   the same (one more rounding of a product is inside it: mean |t - mu||t| >= var)
      shift   mean's + |mu_c| / sigma_c x invstd's + one ulp of the two terms, ULP (|beta| + |mu scale|) / |gamma|"""
    c = t.shape[1]
    flat = t.transpose(0, 1).reshape(c, -1)
    sig, mu = _sigma(st["var"]), st["mean"]
    gamma = st["gamma"].double()
    f_mean = torch.where(sig > 0, ULP * flat.abs().mean(1) / sig.clamp_min(1e-300), torch.full_like(sig, ULP))
    f_inv = ULP * ((flat - mu.view(-1, 1)).abs() * flat.abs()).mean(1) / (st["var"] + st["eps"]) + ULP
    live = gamma != 0
    terms = ULP * (st["beta"].double().abs() + (mu * st["scale"]).abs()) / gamma.abs().clamp_min(1e-300)
    rel_mu = torch.where(sig > 0, mu.abs() / sig.clamp_min(1e-300), torch.zeros_like(sig))
    f_shift = torch.where(live, f_mean * (sig > 0) + rel_mu * f_inv + terms, torch.zeros_like(sig))
    return {"mean": f_mean, "invstd": f_inv, "scale": f_inv, "shift": f_shift}


def own_floors(st):
    """The statistics against those of the kernel's OWN stored output: one ulp of each output"""
    sig, mu, gamma = _sigma(st["var"]), st["mean"], st["gamma"].double()
    f_mean = torch.where(sig > 0, ULP * mu.abs() / sig.clamp_min(1e-300), torch.full_like(sig, ULP))
    one = torch.full_like(sig, ULP)
    f_shift = torch.where(gamma != 0, ULP * (st["shift"].abs() + (mu * st["scale"]).abs()) / gamma.abs().clamp_min(1e-300),
                          torch.zeros_like(sig))
    return {"mean": f_mean, "invstd": one, "scale": one, "shift": f_shift}


def stats_of(y, gamma, beta, eps, dtype):
    """(mean, biased var, invstd, scale, shift, gamma, beta, eps) of y (b,c,m,ns) in dtype, as a dict"""
    y = y.to(dtype)
    mean = y.mean(dim=(0, 2, 3))
    var = y.var(dim=(0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.to(dtype) * invstd
    return {"mean": mean, "var": var, "invstd": invstd, "scale": scale, "shift": beta.to(dtype) - mean * scale,
            "gamma": gamma, "beta": beta, "eps": eps}


def running_errors(got, want, var):
    """got, want = (running_mean, running_var) -> (|rm - t| / (|t| + sigma_c), |rv - t| / |t|), (c) tensors"""
    rm, rv = got[0].double(), got[1].double()
    return (rm - want[0]).abs() / (want[0].abs() + _sigma(var)), (rv - want[1]).abs() / want[1].abs()


def within(e, e32, floor):
    """The rule.  e, e32: a figure of the kernel and of plain fp32 (floats, or per-channel tensors -- the
    yardstick is then plain fp32's WORST channel, so that one lucky fp32 channel cannot fail a kernel channel);
    floor: float or per-channel tensor.  -> (ok, need = max e / bound, e_worst, e32_worst)"""
    if torch.is_tensor(e):
        worst32 = float(e32.max())
        bound = RATIO * worst32 + (floor if torch.is_tensor(floor) else torch.full_like(e, floor))
        exact = bound == 0
        need = torch.where(exact, torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))),
                           e / bound.clamp_min(1e-300))
        return bool((e <= bound).all()), float(need.max()), float(e.max()), worst32
    bound = RATIO * e32 + floor
    return e <= bound, (e / bound if bound > 0 else (0.0 if e == 0 else float("inf"))), e, e32


def with_layer(st, inp, layer):
    """the truth's statistics dict with the layer's gamma, beta and eps beside them"""
    g, be = ("g1", "be1") if layer == 2 else ("g2", "be2")
    out = dict(st)
    out.update(gamma=inp[g], beta=inp[be], eps=inp["eps"])
    return out


def compare_chain(got, p32, tru, inp):
    """Every measure of one run against the truth under the rule.  got / p32: dicts as _layers returns them
    (y2, y3 may be missing in got; stats as dicts or 4-tuples), -> list of (name, ok, need, e, e32)"""
    rows = []
    for layer in (2, 3):
        st = with_layer(tru["stats%d" % layer], inp, layer)
        t = tru["y%d" % layer]
        name = "y%d" % layer
        if got.get(name) is not None:
            eg, ec = tensor_errors(got[name], t, st["var"])
            pg, pc = tensor_errors(p32[name], t, st["var"])
            fg, fc = tensor_floors(t, st["var"])
            rows.append((name + " global",) + within(eg, pg, fg))
            rows.append((name + " channel",) + within(ec, pc, fc))
        tup = lambda s: s if isinstance(s, (tuple, list)) else (s["mean"], s["invstd"], s["scale"], s["shift"])  # noqa: E731
        e, e32 = stat_errors(tup(got["stats%d" % layer]), st), stat_errors(tup(p32["stats%d" % layer]), st)
        fl = stat_floors(t, st)
        for k in ("mean", "invstd", "scale", "shift"):
            rows.append(("%s%d" % (k, layer),) + within(e[k], e32[k], fl[k]))
        run = got.get("running%d" % layer)
        if run is not None:
            er, er32 = running_errors(run, tru["running%d" % layer], st["var"]), \
                running_errors(p32["running%d" % layer], tru["running%d" % layer], st["var"])
            # one ulp of the stored value, and the mean's / variance's floor scaled by the momentum
            rows.append(("running_mean%d" % layer,) + within(er[0], er32[0], ULP + inp["momentum"] * fl["mean"]))
            rows.append(("running_var%d" % layer,) + within(er[1], er32[1], ULP + 2 * inp["momentum"] * fl["invstd"]))
    return rows


# ------------------------------------------------------------------ the kernels' algebra, term by term
SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))   # (weight term, activation term): mlp_frag.h, mfma6
HI_LO, MID_MID = (0, 2), (1, 1)


def bf16_terms(x):
    """x (fp32 tensor) -> its three bf16 terms as float64 tensors, each the truncation of what is left
    (mlp_frag.h: split_terms; pool_gram256_cases.bf16_terms); their sum is x exactly"""
    import numpy as np
    left = np.ascontiguousarray(x.detach().cpu().numpy(), dtype=np.float32)
    out = []
    for _ in range(3):
        t = (left.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
        out.append(torch.from_numpy(t.astype(np.float64)))
        left = left - t   # (exact: the difference fits the format)
    return out


def _split_gemm(w, a, products):
    wt, at = bf16_terms(w), bf16_terms(a)
    y = 0
    for i, j in products:
        y = y + torch.einsum("oc,bcmn->bomn", wt[i], at[j])
    return y


def split_form64(inp, products=SIX):
    """The chain as the kernels evaluate it, in float64 from bf16 terms: layer 1 in fp32 (four FMAs and the
    BatchNorm FMA), each GEMM as the sum of the listed partial products of the operands' bf16 terms, the
    raw outputs and the coefficients rounded to fp32 where the kernels round them.  CPU tensors.
    -> dict as truth64 returns it (no running statistics)"""
    eps = inp["eps"]
    y0 = torch.einsum("oc,bcmn->bomn", inp["w0"], inp["x4"])
    a = torch.relu(y0 * _bc(inp["sc0"], torch.float32) + _bc(inp["sh0"], torch.float32))
    out = {}
    for layer, (w, gamma, beta) in ((2, ("w1", "g1", "be1")), (3, ("w2", "g2", "be2"))):
        y = _split_gemm(inp[w], a, products).float()             # the accumulator is fp32
        st = stats_of(y, inp[gamma], inp[beta], eps, torch.float64)
        out["y%d" % layer] = y
        out["stats%d" % layer] = tuple(st[k].float() for k in ("mean", "invstd", "scale", "shift"))
        a = torch.relu(y.double() * _bc(out["stats%d" % layer][2], torch.float64)
                       + _bc(out["stats%d" % layer][3], torch.float64)).float()   # one rounding: the FMA's
    out["pooled"] = a.amax(3)
    return out


def finalize64(pairs, n_part, gamma, beta, eps, momentum, rm=None, rv=None):
    """chain_finalize_kernel's formula in float64: pairs (parts, c, 2) equal-count (mean, M2) ->
    dict(mean, var, invstd, scale, shift, running_mean, running_var), float64"""
    p = pairs.double()
    parts = p.shape[0]
    n = float(parts) * float(n_part)
    mean = p[:, :, 0].mean(0)
    m2 = p[:, :, 1].sum(0) + n_part * ((p[:, :, 0] - mean.view(1, -1)) ** 2).sum(0)
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * invstd
    out = {"mean": mean, "var": var, "invstd": invstd, "scale": scale, "shift": beta.double() - mean * scale}
    if rm is not None:
        unbiased = m2 / (n - 1.0) if n > 1 else var
        out["running_mean"] = (1 - momentum) * rm.double() + momentum * mean
        out["running_var"] = (1 - momentum) * rv.double() + momentum * unbiased
    return out


# ------------------------------------------------------------------ the first layer
# (b, r): one slice of 4 columns; one slice, its last step partial / full / one step and four columns; two clouds
# of two slices; b > 512: one slice per cloud; 257 slices, the last of 4 columns
FIRST4_SHAPES = ((1, 4), (1, 252), (1, 256), (1, 260), (2, 1028), (600, 8), (1, 131076))
FIRST4_SLICES = {(1, 4): (1, 256), (1, 252): (1, 256), (1, 256): (1, 256), (1, 260): (2, 256),
                 (2, 1028): (5, 256), (600, 8): (1, 256), (1, 131076): (257, 512)}   # (slices, columns per slice)
# first4_moments: b * r = 1, 255, 256, 257, 65535, 65536, 65537 -- one sweep of the 256 x 256 grid and its
# border -- with cloud borders inside a workgroup where b > 1, and (3, 70001)
MOMENT_SHAPES = ((1, 1), (3, 85), (1, 256), (1, 257), (3, 21845), (2, 32768), (1, 65537), (3, 70001))


def first4_slices(b, r):
    """csrc/mlp_first4.hip first4_slices and the launch's columns per slice -> (slices, per)"""
    s = max(1, 512 // max(b, 1))
    per = (-(-r // s) + 255) // 256 * 256
    slices = -(-r // per)
    return slices, (-(-r // slices) + 255) // 256 * 256


def make_moment_input(b, r, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(7919 * seed + 31 * b + r)
    x = torch.randn(b, 4, r, generator=g)
    x[:, 3] = x[:, 3] * 2 + BIG_MEAN
    return x.float().contiguous().to(torch.device(device))


MOMENT_PAIRS = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))


def moments64(x):
    """x (b,4,r) fp32 -> (the 14 moments in float64: 4 sums, then the products in MOMENT_PAIRS' order,
    sum |term| of each)"""
    xd = x.double()
    terms = [xd[:, c] for c in range(4)] + [xd[:, i] * xd[:, j] for i, j in MOMENT_PAIRS]
    return torch.stack([t.sum() for t in terms]), torch.stack([t.abs().sum() for t in terms])


def make_bn_first4(seed=0, device="cpu"):
    """w (64,4) with column 3 damped and row ZERO_ROW1 all zero, gamma (every fifth negative), beta, running
    statistics from random values"""
    g = torch.Generator().manual_seed(4243 * seed + 5)
    w = torch.randn(64, 4, generator=g) * 0.7
    w[:, 3] *= 0.05
    w[ZERO_ROW1] = 0.0
    gamma = torch.rand(64, generator=g) + 0.5
    gamma[::5] *= -1
    ts = (w, gamma, torch.randn(64, generator=g) * 0.3, torch.randn(64, generator=g) * 0.1,
          torch.rand(64, generator=g) + 0.5)
    return tuple(t.float().contiguous().to(torch.device(device)) for t in ts)


def first4_bn_stats(x, w, gamma, beta, rm, rv, momentum, eps, dtype):
    """BatchNorm of y = w x over all b * r columns in dtype -> (stats dict as stats_of, y (b,64,r,1),
    (running_mean, running_var); count = 1: the biased variance (0) enters the running estimate, which is
    what the kernels document -- nn.BatchNorm refuses that input)"""
    y = torch.einsum("oc,bcr->bor", w.to(dtype), x.to(dtype)).unsqueeze(-1)
    st = stats_of(y, gamma, beta, eps, dtype)
    n = x.shape[0] * x.shape[2]
    unbiased = st["var"] * (n / (n - 1.0)) if n > 1 else st["var"]
    run = ((1 - momentum) * rm.to(dtype) + momentum * st["mean"], (1 - momentum) * rv.to(dtype) + momentum * unbiased)
    return st, y, run


def make_first4_inputs(b, r, training, seed=0, device="cpu"):
    """x (b,4,r) with channel 3 at mean 40, w (64,4) (column 3 damped), dz (b,64,r), gamma (every fifth
    negative), beta, and the layer's (scale, shift, mean, invstd, coef) from float64 torch rounded to fp32:
    training -- batch statistics, coef = (gamma invstd, mean of g, mean of g xhat) with g = gate * dz;
    eval -- running statistics, coef = (gamma invstd, 0, 0).  dz is 0 wherever the gate y scale + shift is
    within GATE_ULPS fp32 roundings of zero, so that the gradient depends on no such gate."""
    g = torch.Generator().manual_seed(15485863 * seed + 131 * b + r + (1 if training else 0))
    dev = torch.device(device)
    x = torch.randn(b, 4, r, generator=g)
    x[:, 3] = x[:, 3] * 2 + BIG_MEAN
    w = torch.randn(64, 4, generator=g) * 0.7
    w[:, 3] *= 0.05
    gamma = torch.rand(64, generator=g) + 0.5
    gamma[::5] *= -1
    beta = torch.randn(64, generator=g) * 0.3
    dz = torch.randn(b, 64, r, generator=g)
    x, w, gamma, beta, dz = (t.float().contiguous().to(dev) for t in (x, w, gamma, beta, dz))
    col = lambda v: v.double().view(1, -1, 1)  # noqa: E731
    y = torch.einsum("oc,bcr->bor", w.double(), x.double())
    if training:
        mean = y.mean(dim=(0, 2))
        var = y.var(dim=(0, 2), unbiased=False)
    else:
        mean = (BIG_MEAN * w[:, 3].double() + torch.randn(64, generator=g).to(dev) * 0.1)
        var = (torch.rand(64, generator=g).to(dev).double() + 0.5)
    invstd = 1.0 / torch.sqrt(var + EPS)
    mean, invstd = mean.float(), invstd.float()
    scale = (gamma.double() * invstd.double()).float()
    shift = (beta.double() - mean.double() * scale.double()).float()
    z = y * col(scale) + col(shift)
    mag = torch.einsum("oc,bcr->bor", w.double().abs(), x.double().abs()) * col(scale).abs() + col(shift).abs()
    near = z.abs() <= GATE_ULPS * 2.0 ** -24 * mag
    dz = torch.where(near, torch.zeros((), device=dev), dz).contiguous()
    gsel = torch.where(z > 0, dz.double(), torch.zeros((), dtype=torch.float64, device=dev))
    n = float(b) * float(r)
    a = gamma.double() * invstd.double()
    if training:
        xhat = (y - col(mean)) * col(invstd)
        coef = torch.stack([a, gsel.sum(dim=(0, 2)) / n, (gsel * xhat).sum(dim=(0, 2)) / n], dim=1)
    else:
        coef = torch.stack([a, torch.zeros_like(a), torch.zeros_like(a)], dim=1)
    return {"b": b, "r": r, "training": training, "x": x, "w": w, "dz": dz, "gamma": gamma, "beta": beta,
            "mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "coef": coef.float().contiguous(),
            "excluded": near.double().mean().item(), "var_eval": var}


def check_first4_inputs(inp):
    """no gate the gradient depends on within rounding of zero (dz is 0 there), few of them, both states of
    the gate present"""
    assert inp["excluded"] <= MAX_EXCLUDED, inp["excluded"]
    col = lambda v: v.double().view(1, -1, 1)  # noqa: E731
    y = torch.einsum("oc,bcr->bor", inp["w"].double(), inp["x"].double())
    z = y * col(inp["scale"]) + col(inp["shift"])
    mag = torch.einsum("oc,bcr->bor", inp["w"].double().abs(), inp["x"].double().abs()) * col(inp["scale"]).abs() \
        + col(inp["shift"]).abs()
    used = inp["dz"] != 0
    assert bool((z.abs()[used] > GATE_ULPS * 2.0 ** -24 * mag[used]).all())
    open_ = (z > 0).double().mean().item()
    assert 0.1 < open_ < 0.9, open_
    return {"excluded": inp["excluded"], "open": open_}


def first4_truth64(inp):
    """dW of sum(relu(bn(w x)) * dz) by float64 autograd: conv 1x1 without bias, BatchNorm on batch statistics
    (training) or on the given mean / invstd (eval), ReLU"""
    w = inp["w"].double().requires_grad_(True)
    y = torch.einsum("oc,bcr->bor", w, inp["x"].double())
    col = lambda v: v.double().view(1, -1, 1)  # noqa: E731
    if inp["training"]:
        mean = y.mean(dim=(0, 2), keepdim=True)
        var = y.var(dim=(0, 2), unbiased=False, keepdim=True)
        z = (y - mean) / torch.sqrt(var + EPS) * col(inp["gamma"]) + col(inp["beta"])
    else:
        z = (y - col(inp["mean"])) * col(inp["invstd"]) * col(inp["gamma"]) + col(inp["beta"])
    (torch.relu(z) * inp["dz"].double()).sum().backward()
    return w.grad


def first4_plain_fp32(inp):
    """the yardstick: dy = a (g - c1 - xhat c2) in fp32 from the same fp32 inputs, dW = einsum(dy, x)"""
    with _tf32_off():
        col = lambda v: v.view(1, -1, 1)  # noqa: E731
        x, coef = inp["x"], inp["coef"]
        y = torch.einsum("oc,bcr->bor", inp["w"], x)
        g = torch.where(y * col(inp["scale"]) + col(inp["shift"]) > 0, inp["dz"], torch.zeros((), device=x.device))
        xhat = (y - col(inp["mean"])) * col(inp["invstd"])
        dy = col(coef[:, 0].contiguous()) * (g - col(coef[:, 1].contiguous()) - xhat * col(coef[:, 2].contiguous()))
        return torch.einsum("bor,bcr->oc", dy, x)


def grad_errors(got, truth):
    """-> (||got - truth|| / ||truth||, max |got - truth| / max |truth|)"""
    d = got.double().reshape(truth.shape) - truth
    return (d.norm() / truth.norm()).item(), (d.abs().max() / truth.abs().max()).item()


def grad_floors(truth):
    """one fp32 ulp of the range on every element, in the two measures of grad_errors"""
    return (ULP * truth.abs().max() * truth.numel() ** 0.5 / truth.norm()).item(), ULP
