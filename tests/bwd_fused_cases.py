"""Forms, shapes, inputs, float64 truth and fp32 yardstick for the tests of the one-pass layer backward
(csrc/mlp_bwd_fused.hip: gemm_bwd_fused_kernel in its seven instantiations); no package import.

The kernel is persistent: with T = b * r / tn chunks of tn columns, g = max(1, min(CUs * occ, T / 8))
workgroups and per = ceil(T / g), workgroup i owns the chunks [i * per, min(i * per + per, T)).  A range
may be empty (the workgroup still writes a zero weight partial and zero sums), one chunk or two (the
prologue's clamped look-ahead then re-fetches a chunk it already holds), odd or even (the two LDS
buffers), and may run from one cloud into the next.

  FORMS                           the seven instantiations by name
  fused_shape / supported / workgroups / split / stats_parts / workspace_floats
                                  the host logic of csrc/mlp_bwd_fused.hip, line by line
  pool_lane(ns, tn, col0, seg_c)  the pooled form's lane_g / lane_s / s0 arithmetic
  describe(form, b, groups, ns)   what the ranges of a row of CASES look like
  CASES[form]                     (b, groups, ns, seed); r = groups * ns.  tests/test_bwd_fused_cases.py
                                  proves on the CPU which edges they reach at 256 CUs; the GPU test
                                  asserts that the device's own counts are the mirror's.
  make_inputs(form, ...)          weights / k ** 0.5, BatchNorm weights with every fifth channel negative
                                  on both layers, pool ties in every third group (column 3 a copy of
                                  column 1: the first index wins), a bias of -2 on every seventh channel
                                  of a pooled layer; LIN4: x4 and W0 on a dyadic grid.
  forward64(form, inp)            what the backward consumes -- the raw output y, both layers' statistics
                                  and folded (scale, shift), arg-max, coef -- from torch in float64,
                                  rounded to fp32: no kernel of the project prepares the test's inputs.
                                  rounded=False keeps float64: then reference64 is the module's autograd
                                  to the last bits (the CPU test proves it).
  check_inputs(form, inp, fwd)    the conditions on the data, asserted before anything is compared
  reference64(form, inp, fwd)     dx = W^T P, dw = P Q^T, the layer below's sums, (dgamma, dbeta, coef),
                                  LIN4: G and dw0 -- in float64 on the inputs the kernel reads.  P is
                                  c0 (dz mask - c1 - xhat c2), the BatchNorm + ReLU (+ max) backward in
                                  closed form (csrc/mlp_bn.hip, include/mlp_hip.h); the masks are
                                  fmaf(x, scale, shift) > 0 decided in float64: the product is exact and
                                  the sum keeps its sign.
  plain_fp32(form, inp, fwd)      the same outputs from plain fp32 torch ops: the yardstick
  errors / bound_of / resolution  the two measures, the house rule, the floors from the format
"""
import contextlib

import torch

OP_DIRECT, OP_BNRELU, OP_DY, OP_POOLDY, OP_LIN4 = 0, 1, 2, 3, 4
CUS = 256                     # the CU count the tables were laid out for
EPS = 1e-5
RATIO = 3                     # e(kernel) <= RATIO * e(plain fp32), tests/test_gpu_mlp.py::_grad_bound's margin
ULP = 2.0 ** -23
SHUT_BIAS = -2.0
TWIN_EVERY = 3
LEAST = 8                     # chunks a workgroup gets at least
LIN4_OCC = 1                  # MLP_LIN4_OCC: the LIN4 form's residency (__launch_bounds__).  The GRID of
                              # every form comes from the table's occ: mlp_gemm_backward_fused and
                              # _stats_parts call fused_workgroups(s, .) with the (64,64) row's occ = 2

# fused_shape's table: (m, k, xyz, tn, occ)
TABLE = ((64, 64, 0, 64, 2), (128, 64, 0, 64, 1), (128, 128, 0, 32, 2), (256, 128, 0, 32, 1),
         (128, 131, 3, 32, 1), (128, 259, 3, 32, 1))

# name -> (m, k, pmode, qmode, dq written, sums of the layer below)
FORMS = {
    "bn64": (64, 64, OP_DY, OP_BNRELU, True, True),          # (64,64) over relu(bn(.)), with sums
    "lin4": (64, 64, OP_DY, OP_LIN4, False, True),           # (64,64) T form over the virtual 4 -> 64 layer
    "pool64": (128, 64, OP_POOLDY, OP_BNRELU, True, True),   # pooled, chunk of 64 columns, with sums
    "pool128": (256, 128, OP_POOLDY, OP_BNRELU, True, False),  # pooled, chunk of 32 columns
    "xyz131": (128, 131, OP_DY, OP_DIRECT, True, False),     # direct input, three coordinate rows
    "xyz259": (128, 259, OP_DY, OP_DIRECT, True, False),     # the fp32 instantiation
    "xyz259w": (128, 259, OP_DY, OP_DIRECT, False, False),   # the weight gradient only, bf16 split
}
POOL_NS = {"pool64": (16, 32, 64, 128), "pool128": (16, 32, 64, 96)}
# The forms whose dw gets a third floor, ULP sum_n |P[m][n] Q[k][n]|: one fp32 ulp on every term of the dot
# product, to one side -- below any a-priori bound of an fp32 dot product (u log2(n) sum |pq| at best) and
# the size of what split3 / mfma_x6 may drop of a product (mid lo + lo mid + lo lo < 2^-23 |pq|).
# Pooled (128,64) alone needs it: behind a max pool P is  a dz  at one column in nsample and the small
# dense term  -a (c1 + xhat c2)  everywhere else, Q = relu(.) >= 0, so the dense half of dw is a sum of
# thousands of products of ONE sign, each far below the accumulator -- 512 columns (192 chained bf16
# MFMAs) per workgroup here -- and the matrix pipe's alignment of such addends cuts them to one side
# (the Gram-256 table: -0.014 ulp of the accumulator per instruction).  A float64 evaluation
# of the kernel's own formulas -- folded row constants, fp32 P and Q, six of nine partial products, exact
# sums -- is 1.1e-7 off; the kernel 1.3-1.7e-6 at T = 64 ... 89, plain fp32 3.7-6.4e-7.  Each workgroup's
# partial against float64 over its own columns: -8.5 ... -17.6 ulp along the dense half's sign, the same
# way in every partial.  Measured need of this floor: at most 0.70 (DESIGN.md has every row).
DW_FLOOR = ("pool64",)

_TN64 = (
    (1, 64, 64, 0),       # T = 64: the smallest accepted size, b = 1, ranges of 8
    (1, 73, 64, 0),       # T = 73: per 9, a last range of one chunk
    (1, 130, 32, 0),      # T = 65: per 9, a last range of two chunks
    (1, 89, 64, 0),       # T = 89: g 11, per 9, one empty workgroup below the cap
    (3, 25, 64, 0),       # T = 75: 25 chunks per cloud, both cloud boundaries inside ranges
    (16, 257, 64, 0),     # T = 4112: g = 512 = 2 x 256 CUs, per 9, 55 empty workgroups
)
_TN32 = (
    (1, 64, 32, 0),       # T = 64
    (1, 73, 32, 0),       # T = 73
    (1, 130, 16, 0),      # T = 65
    (1, 89, 32, 0),       # T = 89
    (3, 25, 32, 0),       # T = 75
    (11, 187, 32, 0),     # T = 2057: g = 256 CUs, per 9, 27 empty workgroups, ten cloud boundaries
)
CASES = {
    "bn64": _TN64,
    "lin4": _TN64,
    "pool64": (
        (1, 32, 128, 0),      # T = 64, a group spans two chunks (s0 = 64 in the second)
        (3, 13, 128, 0),      # T = 78: 26 chunks per cloud, boundaries inside ranges, ns = 128
        (1, 292, 16, 0),      # T = 73, four groups per chunk
        (1, 130, 32, 0),      # T = 65, two groups per chunk
        (1, 89, 64, 0),       # T = 89, one group per chunk
        (3, 25, 64, 0),       # T = 75
        (11, 748, 16, 0),     # T = 2057 at the CU count
    ),
    "pool128": (
        (1, 32, 64, 0),       # T = 64, a group spans two chunks
        (2, 13, 96, 0),       # T = 78: a group spans three chunks, 39 chunks per cloud
        (1, 146, 16, 0),      # T = 73, two groups per chunk
        (1, 65, 32, 0),       # T = 65
        (1, 89, 32, 0),       # T = 89
        (3, 25, 32, 0),       # T = 75
        (11, 374, 16, 0),     # T = 2057 at the CU count
    ),
    "xyz131": _TN32,
    "xyz259": _TN32,
    "xyz259w": _TN32,
}


# ------------------------------------------------------------------ the host logic
def fused_shape(m, k):
    """-> dict(m, k, xyz, tn, occ) or None"""
    for row in TABLE:
        if row[0] == m and row[1] == k:
            return dict(zip(("m", "k", "xyz", "tn", "occ"), row))
    return None


def supported(b, m, k, r, pmode, qmode, ns):
    """mlp_gemm_backward_fused_supported"""
    s = fused_shape(m, k)
    if b <= 0 or r <= 0 or s is None:
        return 0
    if r % s["tn"] != 0 or b * (r // s["tn"]) < 64:
        return 0
    if pmode not in (OP_DY, OP_POOLDY):
        return 0
    if pmode == OP_POOLDY and (ns <= 0 or ns % 16 != 0 or r % ns != 0 or (ns % s["tn"] != 0 and s["tn"] % ns != 0)):
        return 0
    if qmode == OP_LIN4:
        return int(m == 64 and k == 64 and pmode == OP_DY)
    if (s["xyz"] != 0) != (qmode == OP_DIRECT):
        return 0
    if qmode not in (OP_DIRECT, OP_BNRELU):
        return 0
    pooled_only = (m, k) in ((128, 64), (256, 128))
    if (m, k) != (128, 128) and pooled_only != (pmode == OP_POOLDY):
        return 0
    return 1


def workgroups(s, T, cus=CUS):
    """fused_workgroups"""
    return max(1, min(cus * s["occ"], T // LEAST))


def split(T, g):
    """-> (per, [(c_lo, c_hi)] * g): the kernel's per / c_lo / c_hi"""
    per = (T + g - 1) // g
    return per, [(i * per, min(i * per + per, T)) for i in range(g)]


def _x6_workgroups(b, m, k, r, cus):
    """mlp_bwd_x6_workgroups: the (128,128) layers' kernel"""
    if (m, k) != (128, 128) or r % 32 != 0 or b <= 0:
        return 0
    return max(1, min(cus, b * (r // 32) // LEAST))


def stats_parts(b, m, k, r, cus=CUS):
    """mlp_gemm_backward_fused_stats_parts"""
    gx = _x6_workgroups(b, m, k, r, cus)
    if gx > 0:
        return gx
    s = fused_shape(m, k)
    if s is None or k != 64 or r % s["tn"] != 0:
        return 0
    return workgroups(s, b * (r // s["tn"]), cus) * 2


def workspace_floats(b, m, k, r, cus=CUS):
    """mlp_gemm_backward_fused_workspace_floats"""
    s = fused_shape(m, k)
    if s is None or r % s["tn"] != 0:
        return 0
    return max(workgroups(s, b * (r // s["tn"]), cus), _x6_workgroups(b, m, k, r, cus)) * m * k


def pool_lane(ns, tn, col0, seg_c):
    """The pooled form's address arithmetic for a lane whose 16 columns start at column col0 + seg_c of a
    cloud (chunk_at: g0, s0; the kernel's lane_g, lane_s) -> (group, first sample): pwin is then
    argmax[group] - first sample, the winner's index among the lane's 16 columns"""
    g0 = col0 // ns
    s0 = col0 - g0 * ns
    lane_g, lane_s = seg_c // ns, seg_c % ns
    return g0 + lane_g, s0 + lane_s


def chunks(form, b, groups, ns):
    m, k = FORMS[form][:2]
    return b * (groups * ns // fused_shape(m, k)["tn"])


def describe(form, b, groups, ns, cus=CUS):
    """-> dict(T, g, per, cap, empty, lengths of the non-empty ranges, last: the last non-empty range's
    length, inside: cloud boundaries strictly inside a range, at_end: those on a range's end)"""
    m, k = FORMS[form][:2]
    s = fused_shape(m, k)
    per_cloud = groups * ns // s["tn"]
    T = b * per_cloud
    g = workgroups(s, T, cus)
    per, ranges = split(T, g)
    live = [(lo, hi) for lo, hi in ranges if lo < hi]
    bounds = [c * per_cloud for c in range(1, b)]
    return {"T": T, "g": g, "per": per, "cap": cus * s["occ"], "empty": g - len(live),
            "lengths": {hi - lo for lo, hi in live}, "last": live[-1][1] - live[-1][0],
            "inside": sum(1 for c in bounds for lo, hi in live if lo < c < hi),
            "at_end": sum(1 for c in bounds for lo, hi in live if c == hi)}


# ------------------------------------------------------------------ inputs
def _bn(c, g):
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::5] *= -1
    return gamma, torch.randn(c, generator=g) * 0.3


def make_inputs(form, b, groups, ns, seed=0, device="cpu"):
    m, k, pmode, qmode, _, _ = FORMS[form]
    g = torch.Generator().manual_seed(100003 * seed + 1009 * b + 10 * groups + ns + 7 * m + k)
    out = {"form": form, "b": b, "groups": groups, "ns": ns, "r": groups * ns, "m": m, "k": k}
    t = {}
    if qmode == OP_LIN4:
        # multiples of 1/8 in [-2, 2] and of 1/16 in [-1, 1]: every product is a multiple of 1/128 below
        # 2, every partial sum of a row below 8 -- exact in fp32 in any order
        t["x4"] = torch.randint(-16, 17, (b, 4, groups, ns), generator=g).float() / 8
        t["w0"] = torch.randint(-16, 17, (64, 4), generator=g).float() / 16
        t["x"] = torch.einsum("kc,bcgn->bkgn", t["w0"].double(), t["x4"].double()).float()
    elif qmode == OP_BNRELU:
        t["x"] = torch.randn(b, k, groups, ns, generator=g) * 1.3 + 0.2
    else:
        t["x"] = torch.randn(b, k, groups, ns, generator=g)
    if pmode == OP_POOLDY:
        t["x"][:, :, ::TWIN_EVERY, 3] = t["x"][:, :, ::TWIN_EVERY, 1]
    t["w"] = torch.randn(m, k, generator=g) / k ** 0.5
    if qmode != OP_DIRECT:
        t["gx"], t["bex"] = _bn(k, g)
    t["g"], t["be"] = _bn(m, g)
    if pmode == OP_POOLDY:
        t["be"][2::7] += SHUT_BIAS
        t["dz"] = torch.randn(b, m, groups, generator=g)
    else:
        t["dz"] = torch.randn(b, m, groups, ns, generator=g)
    for name, v in t.items():
        out[name] = v.float().contiguous().to(torch.device(device))
    return out


def _col(v):
    return v.double().view(1, -1, 1)


def _stats64(y, gamma, beta, rounded):
    mean = y.mean(dim=(0, 2))
    invstd = 1.0 / torch.sqrt(y.var(dim=(0, 2), unbiased=False) + EPS)
    if rounded:
        mean, invstd = mean.float().double(), invstd.float().double()
    scale = gamma.double() * invstd
    if rounded:
        scale = scale.float().double()
    shift = beta.double() - mean * scale
    return mean, invstd, scale, shift


def _keep(v, rounded):
    return v.float().contiguous() if rounded else v.contiguous()


def forward64(form, inp, rounded=True):
    """-> dict: y (b,m,groups,ns) the layer's raw output, mean / invstd / sc / sh of its BatchNorm, coef
    (m,3) = (gamma invstd, sum g / N, sum g xhat / N) with g the gated incoming gradient, argmax (pooled);
    meanx / invx / scx / shx of the layer below (not for a direct input).  fp32 (int32) when `rounded`, as
    the kernels read them; every later quantity is computed from the rounded earlier ones."""
    m, k, pmode, qmode, _, _ = FORMS[form]
    b, groups, ns, r = inp["b"], inp["groups"], inp["ns"], inp["r"]
    x = inp["x"].double().view(b, k, r)
    out = {}
    if qmode != OP_DIRECT:
        meanx, invx, scx, shx = _stats64(x, inp["gx"], inp["bex"], rounded)
        a = torch.relu(x * _col(scx) + _col(shx))
        out.update(meanx=meanx, invx=invx, scx=scx, shx=shx)
    else:
        a = x
    y = torch.einsum("mk,bkr->bmr", inp["w"].double(), a)
    del a
    if rounded:
        y = y.float().double()
    if pmode == OP_POOLDY:   # (the twin columns' outputs are the same number)
        y4 = y.view(b, m, groups, ns)
        y4[:, :, ::TWIN_EVERY, 3] = y4[:, :, ::TWIN_EVERY, 1]
    mean, invstd, sc, sh = _stats64(y, inp["g"], inp["be"], rounded)
    z = y * _col(sc) + _col(sh)
    xhat = (y - _col(mean)) * _col(invstd)
    n = float(b) * float(r)
    zero = torch.zeros((), dtype=torch.float64, device=y.device)
    if pmode == OP_POOLDY:
        z4 = z.view(b, m, groups, ns)
        pos = torch.arange(ns, device=z.device).view(1, 1, 1, ns).expand_as(z4)
        first = torch.where(z4 == z4.amax(3, keepdim=True), pos, torch.full_like(pos, ns)).amin(3)
        zw = torch.gather(z4, 3, first.unsqueeze(-1)).squeeze(-1)
        xw = torch.gather(xhat.view(b, m, groups, ns), 3, first.unsqueeze(-1)).squeeze(-1)
        gsel = torch.where(zw > 0, inp["dz"].double(), zero)
        s1, s2 = gsel.sum(dim=(0, 2)), (gsel * xw).sum(dim=(0, 2))
        out["argmax"] = first.int().contiguous()
    else:
        gd = torch.where(z > 0, inp["dz"].double().view(b, m, r), zero)
        s1, s2 = gd.sum(dim=(0, 2)), (gd * xhat).sum(dim=(0, 2))
    coef = torch.stack([inp["g"].double() * invstd, s1 / n, s2 / n], dim=1)
    out.update(y=y.view(b, m, groups, ns), mean=mean, invstd=invstd, sc=sc, sh=sh, coef=coef)
    return {name: (v if v.dtype == torch.int32 else _keep(v, rounded)) for name, v in out.items()}


def _operands64(form, inp, fwd):
    """-> (P (b,m,r), Q (b,k,r), gate of the layer below or None, x (b,k,r)) in float64"""
    m, k, pmode, qmode, _, _ = FORMS[form]
    b, groups, ns, r = inp["b"], inp["groups"], inp["ns"], inp["r"]
    y = fwd["y"].double().view(b, m, r)
    open_ = (y * _col(fwd["sc"]) + _col(fwd["sh"])) > 0
    zero = torch.zeros((), dtype=torch.float64, device=y.device)
    if pmode == OP_POOLDY:
        dz = torch.zeros(b, m, groups, ns, dtype=torch.float64, device=y.device)
        dz.scatter_(3, fwd["argmax"].long().unsqueeze(-1), inp["dz"].double().unsqueeze(-1))
        dz = dz.view(b, m, r)
    else:
        dz = inp["dz"].double().view(b, m, r)
    coef = fwd["coef"].double()
    xhat = (y - _col(fwd["mean"])) * _col(fwd["invstd"])
    P = _col(coef[:, 0]) * (torch.where(open_, dz, zero) - _col(coef[:, 1]) - xhat * _col(coef[:, 2]))
    x = inp["x"].double().view(b, k, r)
    if qmode == OP_DIRECT:
        return P, x, None, x
    zx = x * _col(fwd["scx"]) + _col(fwd["shx"])
    return P, torch.relu(zx), zx > 0, x


def reference64(form, inp, fwd):
    """-> dict of float64 tensors: dx (b,k,r), dw (m,k); with a BatchNorm layer below also s_one = sum g,
    s_xhat = sum g xhat (g = dx where that layer's ReLU is open), coef (k,3) = (gamma invstd, s_one / N,
    s_xhat / N) -- dgamma is s_xhat, dbeta is s_one; LIN4 also G (64,4) = sum g x4^T and dw0 (64,4), the
    virtual layer's weight gradient by autograd through its BatchNorm on batch statistics"""
    m, k, pmode, qmode, _, _ = FORMS[form]
    b, r = inp["b"], inp["r"]
    P, Q, gate, x = _operands64(form, inp, fwd)
    out = {"dx": torch.einsum("mk,bmr->bkr", inp["w"].double(), P), "dw": torch.einsum("bmr,bkr->mk", P, Q)}
    del P, Q
    if gate is None:
        return out
    gq = torch.where(gate, out["dx"], torch.zeros((), dtype=torch.float64, device=x.device))
    xhat = (x - _col(fwd["meanx"])) * _col(fwd["invx"])
    n = float(b) * float(r)
    out["s_one"], out["s_xhat"] = gq.sum(dim=(0, 2)), (gq * xhat).sum(dim=(0, 2))
    out["coef"] = torch.stack([inp["gx"].double() * fwd["invx"].double(), out["s_one"] / n, out["s_xhat"] / n], dim=1)
    if qmode == OP_LIN4:
        x4 = inp["x4"].double().view(b, 4, r)
        out["G"] = torch.einsum("bkr,bcr->kc", gq, x4)
        del gq, xhat
        w0 = inp["w0"].double().requires_grad_(True)
        y0 = torch.einsum("kc,bcr->bkr", w0, x4)
        mean = y0.mean(dim=(0, 2), keepdim=True)
        var = y0.var(dim=(0, 2), unbiased=False, keepdim=True)
        a0 = torch.relu((y0 - mean) / torch.sqrt(var + EPS) * _col(inp["gx"]) + _col(inp["bex"]))
        a0.backward(out["dx"])
        out["dw0"] = w0.grad
    return out


@contextlib.contextmanager
def _tf32_off():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old


def _c32(v):
    return v.view(1, -1, 1)


def plain_fp32(form, inp, fwd):
    """The outputs of reference64 from plain fp32 torch ops on the same fp32 inputs: the operand
    c0 (dz mask - c1 - xhat c2) element by element, two matmuls, fp32 sums; LIN4: dw0 = dy0 x4^T with dy0
    the virtual layer's BatchNorm + ReLU backward from the fp32 coefficients"""
    m, k, pmode, qmode, _, _ = FORMS[form]
    b, groups, ns, r = inp["b"], inp["groups"], inp["ns"], inp["r"]
    with _tf32_off():
        y = fwd["y"].view(b, m, r)
        zero = torch.zeros((), device=y.device)
        open_ = (y * _c32(fwd["sc"]) + _c32(fwd["sh"])) > 0
        if pmode == OP_POOLDY:
            dz = torch.zeros(b, m, groups, ns, device=y.device)
            dz.scatter_(3, fwd["argmax"].long().unsqueeze(-1), inp["dz"].unsqueeze(-1))
            dz = dz.view(b, m, r)
        else:
            dz = inp["dz"].view(b, m, r)
        coef = fwd["coef"]
        xhat = (y - _c32(fwd["mean"])) * _c32(fwd["invstd"])
        P = _c32(coef[:, 0].contiguous()) * (torch.where(open_, dz, zero) - _c32(coef[:, 1].contiguous())
                                             - xhat * _c32(coef[:, 2].contiguous()))
        del xhat, dz, open_
        x = inp["x"].view(b, k, r)
        if qmode == OP_DIRECT:
            Q, gate = x, None
        else:
            zx = x * _c32(fwd["scx"]) + _c32(fwd["shx"])
            Q, gate = torch.relu(zx), zx > 0
        out = {"dx": torch.matmul(inp["w"].t(), P), "dw": torch.matmul(P, Q.transpose(1, 2)).sum(dim=0)}
        del P, Q
        if gate is None:
            return out
        gq = torch.where(gate, out["dx"], zero)
        xhat = (x - _c32(fwd["meanx"])) * _c32(fwd["invx"])
        n = float(b) * float(r)
        out["s_one"], out["s_xhat"] = gq.sum(dim=(0, 2)), (gq * xhat).sum(dim=(0, 2))
        out["coef"] = torch.stack([inp["gx"] * fwd["invx"], out["s_one"] / n, out["s_xhat"] / n], dim=1)
        if qmode == OP_LIN4:
            x4 = inp["x4"].view(b, 4, r)
            out["G"] = torch.matmul(gq, x4.transpose(1, 2)).sum(dim=0)
            c = out["coef"]
            dy0 = _c32(c[:, 0].contiguous()) * (gq - _c32(c[:, 1].contiguous()) - xhat * _c32(c[:, 2].contiguous()))
            out["dw0"] = torch.matmul(dy0, x4.transpose(1, 2)).sum(dim=0)
        return out


# ------------------------------------------------------------------ conditions on the data
MIN_SHARE = 0.02
LIN4_MARGIN = 1e-6            # LIN4: |bn0(y0)| of the virtual layer on float64 statistics, values of order 1


def check_inputs(form, inp, fwd, coverage=True):
    """The conditions on the data -> dict of measured shares (coverage=False: a shape too small for the
    winners to reach every column; the CPU test of the closed forms has such).
    * Every fifth BatchNorm weight is negative, on both layers.
    * The layer's ReLU is open in a share of its entries and shut in a share; so is the ReLU below.
    * Pooled: the winners are the first maxima, no later twin wins, and the winners whose ReLU is open
      take every column of a chunk that they can.
    * LIN4: every partial sum of lin4()'s chain is an fp32 number (the kernel's recomputed rows are the
      stored ones, bit for bit), and no pre-activation of the virtual layer is within LIN4_MARGIN of zero on
      float64 statistics (the autograd truth of dw0 then takes the gates the kernel takes)."""
    m, k, pmode, qmode, _, _ = FORMS[form]
    b, groups, ns, r = inp["b"], inp["groups"], inp["ns"], inp["r"]
    tn = fused_shape(m, k)["tn"]
    info = {}
    assert bool((inp["g"][::5] < 0).all()) and int((inp["g"] < 0).sum()) == (m + 4) // 5
    y = fwd["y"].double().view(b, m, groups, ns)
    z = y * fwd["sc"].double().view(1, -1, 1, 1) + fwd["sh"].double().view(1, -1, 1, 1)
    if pmode == OP_POOLDY:
        am = fwd["argmax"].long()
        zw = torch.gather(z, 3, am.unsqueeze(-1)).squeeze(-1)
        assert bool((zw == z.amax(3)).all())
        pos = torch.arange(ns, device=z.device).view(1, 1, 1, ns)
        assert not bool(((z == zw.unsqueeze(-1)) & (pos < am.unsqueeze(-1))).any()), "an earlier maximum"
        assert not bool((am[:, :, ::TWIN_EVERY] == 3).any()), "a later twin won"
        twins = am[:, :, ::TWIN_EVERY]
        if 2 * twins.numel() >= 16 * ns:   # (a twin wins one group in ns / 2: expect 16 and more)
            assert bool((twins == 1).any()), "no tie was ever decided"
        possible = {(j * ns + p) % tn for j in range(groups) for p in range(ns)
                    if not (j % TWIN_EVERY == 0 and p == 3)}
        col = (am + ns * torch.arange(groups, device=am.device).view(1, 1, groups)) % tn
        assert not coverage or set(col[zw > 0].unique().tolist()) == possible
        info["open"] = (zw > 0).double().mean().item()
    else:
        info["open"] = (z > 0).double().mean().item()
    assert MIN_SHARE < info["open"] < 1 - MIN_SHARE, info["open"]
    del z
    if qmode != OP_DIRECT:
        assert bool((inp["gx"][::5] < 0).all()) and int((inp["gx"] < 0).sum()) == (k + 4) // 5
        x = inp["x"].double().view(b, k, r)
        gate = (x * _col(fwd["scx"]) + _col(fwd["shx"])) > 0
        info["open_below"] = gate.double().mean().item()
        assert MIN_SHARE < info["open_below"] < 1 - MIN_SHARE
    if qmode == OP_LIN4:
        x4, w0 = inp["x4"].double().view(b, 4, r), inp["w0"].double()
        acc = torch.zeros(b, 64, r, dtype=torch.float64, device=x4.device)
        for c in range(4):   # lin4(): w.x x0, then one fused multiply-add per channel
            acc = acc + w0[:, c].view(1, -1, 1) * x4[:, c].unsqueeze(1)
            assert torch.equal(acc.float().double(), acc), "a partial sum of lin4() is not an fp32 number"
        assert torch.equal(acc, x), "x is not the virtual layer's output"
        mean = x.mean(dim=(0, 2), keepdim=True)
        var = x.var(dim=(0, 2), unbiased=False, keepdim=True)
        z0 = (x - mean) / torch.sqrt(var + EPS) * _col(inp["gx"]) + _col(inp["bex"])
        info["lin4_margin"] = z0.abs().min().item()
        assert info["lin4_margin"] > LIN4_MARGIN, "a gate of the virtual layer within %g of zero: take another seed" % LIN4_MARGIN
        assert bool(((z0 > 0) == gate).all())
    return info


# ------------------------------------------------------------------ measures, bound, floors
def errors(got, truth):
    """-> (||got - truth|| / ||truth||, max |got - truth| / max |truth|)"""
    d = got.double().reshape(truth.shape) - truth
    return (d.norm() / truth.norm()).item(), (d.abs().max() / truth.abs().max()).item()


def bound_of(e32, floor=(0.0, 0.0)):
    """what the kernel may err by: RATIO times the fp32 yardstick's own error, per measure, plus a floor"""
    return tuple(RATIO * e + f for e, f in zip(e32, floor))


def _floor(f, truth):
    return (f.norm() / truth.norm()).item(), (f.max() / truth.abs().max()).item()


def resolution(form, inp, fwd, ref):
    """What ONE fp32 ulp on every element of dx is worth in the quantities summed over it, in the two
    measures of errors(): for s_one ULP sum gate |dx| per channel, for s_xhat the same times |xhat|, for
    the coefficient columns 1 and 2 the same over N; LIN4: for G ULP sum gate |dx| |x4|, and for dw0 that
    and the two sums through first4_combine's formula  a (G - c1 X1 - c2 invstd (W0 S - mean X1)).
    An error of dx with one sign in every column goes into a sum whole, however small it is element by
    element (the Gram-256 table: the matrix pipe leaves one), and a BatchNorm backward's sums
    cancel to a small part of sum |dx|.
    For the forms of DW_FLOOR also "dw": ULP sum_n |P Q| per element, one ulp on every TERM of the weight
    gradient's dot product (see DW_FLOOR).  -> {name: (floor on rel-L2, floor on max / range)}"""
    m, k, pmode, qmode, _, _ = FORMS[form]
    out = {}
    if form in DW_FLOOR:
        P, Q, _, _ = _operands64(form, inp, fwd)
        out["dw"] = _floor(ULP * torch.einsum("bmr,bkr->mk", P.abs(), Q.abs()), ref["dw"])
        del P, Q
    if qmode == OP_DIRECT:
        return out
    b, r = inp["b"], inp["r"]
    x = inp["x"].double().view(b, k, r)
    gate = (x * _col(fwd["scx"]) + _col(fwd["shx"])) > 0
    mag = torch.where(gate, ref["dx"].abs(), torch.zeros((), dtype=torch.float64, device=x.device))
    xhat = ((x - _col(fwd["meanx"])) * _col(fwd["invx"])).abs()
    f1, f2 = ULP * mag.sum(dim=(0, 2)), ULP * (mag * xhat).sum(dim=(0, 2))
    out.update(s_one=_floor(f1, ref["s_one"]), s_xhat=_floor(f2, ref["s_xhat"]))
    if qmode == OP_LIN4:
        x4 = inp["x4"].double().view(b, 4, r)
        fg = ULP * torch.einsum("bkr,bcr->kc", mag, x4.abs())
        out["G"] = _floor(fg, ref["G"])
        n = float(b) * float(r)
        x1 = x4.sum(dim=(0, 2))                                  # (4)
        ws = inp["w0"].double() @ torch.einsum("bcr,bdr->cd", x4, x4)   # (64,4)
        a, inv, mean = ref["coef"][:, 0].abs().view(-1, 1), fwd["invx"].double().view(-1, 1), fwd["meanx"].double().view(-1, 1)
        fd = a * (fg + f1.view(-1, 1) / n * x1.abs().view(1, -1) + f2.view(-1, 1) / n * (inv * (ws - mean * x1.view(1, -1))).abs())
        out["dw0"] = _floor(fd, ref["dw0"])
    return out
