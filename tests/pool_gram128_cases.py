"""Shapes, inputs, float64 truth and fp32 yardstick for the tests of SA1's 64 -> 128 Gram backward
(csrc/mlp_pool_gram.hip: prep, the persistent pass, reduce, dw); no package import.  The vocabulary is
tests/pool_gram256_cases.py's, whose dimension-free helpers are imported, not copied.

The pass is persistent: with T = b * r / 32 chunks of 32 columns, g = max(1, min(CUs, T / 8)) workgroups
and per = ceil(T / g), workgroup i owns the chunks [i * per, min(i * per + per, T)).  A range may be
empty (the workgroup still writes its zero partials), one chunk (the look-ahead re-stages the chunk
itself), odd (the last chunk runs on buffer 0 alone), even, and may run from one cloud into the next.
What this pass has that no other kernel has is the sparse gradient S as an LDS image: every (channel,
group) thread writes one entry at [channel][winner's column] when a chunk is staged and clears it one
chunk later; the entry goes to the padding column 32 when the winner lies outside the chunk (ns = 64: a
group spans two chunks, and with an odd per its halves belong to different workgroups) or the pooled
ReLU is shut; ns = 16 puts two groups in one chunk.  The reduce kernel sums the g partials four at a
time per slice of eight while p + 24 < g, one at a time after that.

  covers(b, r, ns)                gram_covers
  describe(b, m, ns, cus)         what the ranges look like for a row of CASES: T, g, per, empty,
                                  lengths, crossing, group_split (ns = 64: range boundaries inside a
                                  group), reduce_form (the (four-wide, single) iterations of the slices)
  workspace_floats(...)           mlp_pool_gram_workspace_floats' formula at (128, 64)
  CASES                           (b, groups m, ns, seed); r = m * ns.  tests/test_pool_gram128_cases.py
                                  proves on the CPU that they reach every edge above at 256 CUs; the
                                  GPU test asserts that the device's own counts are the mirror's.
  SPARSE_ONLY                     the rows (one per ns) that also run with coef3's c1 = c2 = 0
  make_inputs(b, m, ns, seed)     as pool_gram256_cases.make_inputs, at (128, 64)
  forward64(inp, sparse_only)     what the backward consumes, from torch in float64, rounded to fp32: no
                                  kernel of the project prepares the test's inputs.  sparse_only: c1 =
                                  c2 = 0 in coef3 (what eval-mode BatchNorm gives): q = p = 0, M3 = v = 0,
                                  and the truth is dq = W3^T S, dW = S a2^T: the sparse image alone.
  check_inputs(inp, fwd)          the conditions on the data, asserted before anything is compared.
  reference64(inp, fwd)           the reference module's layer in float64 with autograd
  plain_fp32(inp, fwd)            the same outputs from plain fp32 torch ops
  sums_resolution(inp, fwd, ref)  what one fp32 ulp per element of dq is worth in the sums over it
  within(name, e, e32, res)       the GPU test's rule: e <= RATIO * e32 + floor, per measure
  gram_form64(inp, fwd, ...)      the pass's own formulas in float64 numpy, the operands cut to `terms`
                                  bf16 terms, the listed partial products kept
"""
import contextlib

import torch

from pool_gram256_cases import (CUS, EPS, GATE_ULPS, MIN_SHARE, POOL_MARGIN, RATIO, SHUT_BIAS, TWIN_EVERY, ULP,
                                bf16_terms, bound_of, errors, split)

__all__ = ["CUS", "RATIO", "ULP", "bf16_terms", "bound_of", "errors", "split"]

K_IN, M_OUT, CHUNK = 64, 128, 32
LEAST = 8                     # chunks per workgroup, at least (gram_workgroups)
MIN_CHUNKS = 64               # gram_covers: fewer chunks are not worth the pass
SUMS = K_IN * K_IN + K_IN + M_OUT * K_IN
OUTPUTS = ("dq", "dw", "s_xhat", "s_one", "coef0")

# (b, groups m, ns, seed): the smallest shapes that reach each edge at 256 CUs.  The seeds are those at
# which check_inputs holds (no ReLU gate of either layer within rounding of zero).
CASES = (
    (1, 128, 16, 0),     # T = 64: the smallest covered shape, two groups per chunk
    (1, 64, 32, 0),      # T = 64
    (1, 32, 64, 0),      # T = 64, two chunks per group
    (1, 146, 16, 0),     # T = 73 = 8 * 9 + 1: a last range of one chunk
    (1, 73, 32, 0),      # T = 73
    (1, 41, 64, 0),      # T = 82 = 9 * 9 + 1: one chunk at the end, 5 groups split between workgroups
    (3, 54, 16, 0),      # T = 81: one empty workgroup
    (3, 27, 32, 0),      # T = 81
    (5, 13, 32, 0),      # T = 65: 4 ranges cross clouds, a last range of two
    (3, 11, 64, 0),      # T = 66: 2 crossing, 4 groups split
    (3, 67, 32, 0),      # T = 201: 25 partials: slice 0 sums four at a time, the others one at a time
    (5, 21, 64, 0),      # T = 210: 12 groups split, 3 crossing
    (3, 88, 32, 0),      # T = 264: 33 partials: slice 0 mixes both loops
    (2, 514, 64, 0),     # T = 2056: the grid at the CU count, 114 groups split
    (2, 2056, 16, 1),    # T = 2056
    (2, 2056, 32, 5),    # T = 4112: both lengths odd, every slice four at a time
)
SPARSE_ONLY = ((1, 146, 16), (1, 73, 32), (1, 41, 64))


# ------------------------------------------------------------------ the split
def covers(b, r, ns):
    """gram_covers"""
    return b > 0 and r > 0 and r % 32 == 0 and ns in (16, 32, 64) and r % ns == 0 and b * (r // 32) >= MIN_CHUNKS


def chunks(b, m, ns):
    return b * (m * ns // CHUNK)


def reduce_form(parts):
    """-> the set of (four-wide iterations, single iterations) of pool_gram_reduce_kernel's two loops over
    its eight slices"""
    forms = set()
    for sl in range(8):
        p, wide, single = sl, 0, 0
        while p + 24 < parts:
            wide, p = wide + 1, p + 32
        while p < parts:
            single, p = single + 1, p + 8
        forms.add((wide, single))
    return forms


def describe(b, m, ns, cus=CUS):
    """-> dict(T, g, per, empty, lengths: set of the non-empty ranges' lengths, crossing: ranges whose
    chunks lie in more than one cloud, group_split: for ns = 64 the inner range boundaries at an odd
    chunk -- the two halves of that group go to different workgroups -- else 0, reduce_form)"""
    per_cloud = m * ns // CHUNK
    T = b * per_cloud
    g, per, ranges = split(T, LEAST, cus)
    live = [(lo, hi) for lo, hi in ranges if lo < hi]
    return {"T": T, "g": g, "per": per, "empty": len(ranges) - len(live),
            "lengths": {hi - lo for lo, hi in live},
            "crossing": sum(1 for lo, hi in live if lo // per_cloud != (hi - 1) // per_cloud),
            "group_split": sum(1 for lo, hi in live if ns == 64 and hi < T and hi % 2),
            "reduce_form": reduce_form(g)}


def workspace_floats(b, m, ns, cus=CUS):
    """mlp_pool_gram_workspace_floats: qp, M3, v, the partials per workgroup, the sums as doubles, 16 spare"""
    g = split(chunks(b, m, ns), LEAST, cus)[0]
    return 256 + 4096 + 64 + g * (4096 + 64 + 8192) + 2 * SUMS + 16


# ------------------------------------------------------------------ inputs
def make_inputs(b, m, ns, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(200003 * seed + 1013 * b + 10 * m + ns)
    y2 = torch.randn(b, K_IN, m, ns, generator=g) * 1.3 + 0.2
    y2[:, :, ::TWIN_EVERY, 3] = y2[:, :, ::TWIN_EVERY, 1]
    w3 = torch.randn(M_OUT, K_IN, generator=g) / K_IN ** 0.5

    def bn(c):
        gamma = torch.rand(c, generator=g) + 0.5
        gamma[::5] *= -1
        return gamma, torch.randn(c, generator=g) * 0.3

    g2, be2 = bn(K_IN)
    g3, be3 = bn(M_OUT)
    be3[2::7] += SHUT_BIAS
    dpooled = torch.randn(b, M_OUT, m, generator=g)
    dev = torch.device(device)
    out = {"b": b, "m": m, "ns": ns, "r": m * ns}
    for name, t in (("y2", y2), ("w3", w3), ("g2", g2), ("be2", be2), ("g3", g3), ("be3", be3),
                    ("dpooled", dpooled)):
        out[name] = t.float().contiguous().to(dev)
    return out


def _stats64(y, gamma, beta):
    """y (b,c,r) float64 -> fp32 (mean, invstd, scale, shift) of a BatchNorm on batch statistics"""
    mean = y.mean(dim=(0, 2))
    invstd = 1.0 / torch.sqrt(y.var(dim=(0, 2), unbiased=False) + EPS)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    return tuple(t.float().contiguous() for t in (mean, invstd, scale, shift))


def _col(v):
    return v.double().view(1, -1, 1)


def forward64(inp, sparse_only=False):
    """-> dict of fp32 tensors: mean2, invstd2, sc2, sh2, mean3, invstd3, sc3, sh3, argmax (int32), ymax,
    coef3 (128,3) = (gamma invstd, sum g / N, sum g xhat / N) with g the gated pooled gradient -- or
    (gamma invstd, 0, 0) with sparse_only"""
    b, m, ns, r = inp["b"], inp["m"], inp["ns"], inp["r"]
    y2 = inp["y2"].double().view(b, K_IN, r)
    mean2, invstd2, sc2, sh2 = _stats64(y2, inp["g2"], inp["be2"])
    a2 = torch.relu(y2 * _col(sc2) + _col(sh2))
    y3 = torch.einsum("ok,bkr->bor", inp["w3"].double(), a2)
    del a2
    mean3, invstd3, sc3, sh3 = _stats64(y3, inp["g3"], inp["be3"])
    y3 = y3.view(b, M_OUT, m, ns)
    y3[:, :, ::TWIN_EVERY, 3] = y3[:, :, ::TWIN_EVERY, 1]   # (the twin columns' outputs are the same number)
    z = y3 * sc3.double().view(1, -1, 1, 1) + sh3.double().view(1, -1, 1, 1)
    pos = torch.arange(ns, device=z.device).view(1, 1, 1, ns).expand_as(z)
    first = torch.where(z == z.amax(3, keepdim=True), pos, torch.full_like(pos, ns)).amin(3)
    del z, pos
    ymax = torch.gather(y3, 3, first.unsqueeze(-1)).squeeze(-1).float().contiguous()
    del y3
    open_ = (ymax.double() * _col(sc3) + _col(sh3)) > 0   # the kernel's gate, fmaf(ymax, sc3, sh3) > 0
    gsel = torch.where(open_, inp["dpooled"].double(), torch.zeros((), dtype=torch.float64, device=ymax.device))
    xhat = (ymax.double() - _col(mean3)) * _col(invstd3)
    n = float(b) * float(r)
    coef3 = torch.stack([inp["g3"].double() * invstd3.double(), gsel.sum(dim=(0, 2)) / n,
                         (gsel * xhat).sum(dim=(0, 2)) / n], dim=1)
    if sparse_only:
        coef3[:, 1:] = 0.0
    return {"mean2": mean2, "invstd2": invstd2, "sc2": sc2, "sh2": sh2, "mean3": mean3, "invstd3": invstd3,
            "sc3": sc3, "sh3": sh3, "argmax": first.int().contiguous(), "ymax": ymax,
            "coef3": coef3.float().contiguous(), "sparse_only": bool(sparse_only)}


def _open(inp, fwd):
    return (fwd["ymax"].double() * _col(fwd["sc3"]) + _col(fwd["sh3"])) > 0


def sparse_columns(inp, fwd):
    """-> int64 (128 channels, threads per channel, T): the chunk column at which the thread (channel, lgi)
    writes its entry of the sparse image in chunk c, in the kernel's order of the chunks; 32 (the padding
    column) where the pooled ReLU is shut or, with ns = 64, the winner lies in the group's other half"""
    b, m, ns = inp["b"], inp["m"], inp["ns"]
    am = fwd["argmax"].long()
    pad = torch.full((), CHUNK, dtype=torch.int64, device=am.device)
    am = torch.where(_open(inp, fwd), am, torch.full_like(am, 2 * ns + CHUNK))   # (shut: in no half, no chunk)
    if ns == 64:
        halves = torch.stack([torch.where((am >= CHUNK * h) & (am < CHUNK * h + CHUNK), am - CHUNK * h, pad)
                              for h in (0, 1)], dim=3)                       # (b, 128, m, 2): chunk 2 j + h
        return halves.permute(1, 0, 2, 3).reshape(M_OUT, 1, b * m * 2)
    if ns == 32:
        return torch.where(am < ns, am, pad).permute(1, 0, 2).reshape(M_OUT, 1, b * m)
    col = torch.where(am < ns, am + ns * (torch.arange(m, device=am.device) % 2).view(1, 1, m), pad)
    return col.view(b, M_OUT, m // 2, 2).permute(1, 3, 0, 2).reshape(M_OUT, 2, b * m // 2)


def check_inputs(inp, fwd):
    """The conditions on the data (asserted, not excused afterwards; no row skips one) -> dict of the
    measured figures.
    * No layer-2 pre-activation y2 sc2 + sh2 within GATE_ULPS fp32 roundings of zero: the kernel's fused
      multiply-add has the sign of the exact value, and so does any fp32 evaluation that far from zero.
    * No pooled pre-activation of layer 3 within POOL_MARGIN of zero, in float64 on float64 statistics:
      the kernel decides on fmaf(fp32 ymax, fp32 scale, fp32 shift), some 1e-6 away from that.
    * The winners whose ReLU is open take every one of a chunk's 32 columns, 0 and 31 included; with
      ns = 64 in both halves of a group, with ns = 16 in both groups of a chunk.
    * Some (channel, thread) has open winners at one column in two consecutive chunks of one workgroup's
      range (the clear in one buffer and the write in the other meet at one column), and some at one
      column in the chunks c and c + 2 (the clear and the write that follows it hit one address).
    * The ReLU behind the pool is shut in a share of the (channel, group) entries and open in a share."""
    b, m, ns, r = inp["b"], inp["m"], inp["ns"], inp["r"]
    y2 = inp["y2"].double().view(b, K_IN, r)
    prod = y2 * _col(fwd["sc2"])
    z2 = prod + _col(fwd["sh2"])
    eps32 = 2.0 ** -24
    slack = (z2.abs() - GATE_ULPS * eps32 * (prod.abs() + _col(fwd["sh2"]).abs())).min().item()
    assert slack > 0, "a layer-2 ReLU gate within %d roundings of zero: take another seed" % GATE_ULPS
    a2 = torch.relu(z2)
    del prod, z2
    y3 = torch.einsum("ok,bkr->bor", inp["w3"].double(), a2)
    mean = y3.mean(dim=(0, 2), keepdim=True)
    var = y3.var(dim=(0, 2), unbiased=False, keepdim=True)
    z3 = ((y3 - mean) / torch.sqrt(var + EPS) * _col(inp["g3"]) + _col(inp["be3"])).view(b, M_OUT, m, ns)
    del y3
    am = fwd["argmax"].long()
    zw = torch.gather(z3, 3, am.unsqueeze(-1)).squeeze(-1)
    margin = zw.abs().min().item()
    assert margin > POOL_MARGIN, "a pooled ReLU gate within %g of zero: take another seed" % POOL_MARGIN
    open_ = _open(inp, fwd)
    assert bool((open_ == (zw > 0)).all())
    assert float((zw - z3.amax(3)).abs().max()) <= 1e-9   # the winners are the maxima
    assert not bool((am[:, :, ::TWIN_EVERY] == 3).any()), "a later twin won"
    cols = sparse_columns(inp, fwd)
    T = chunks(b, m, ns)
    assert cols.shape == (M_OUT, CHUNK // ns if ns < CHUNK else 1, T)
    assert set(cols.unique().tolist()) == set(range(CHUNK + 1))   # every column, and the padding
    if ns == 64:
        for h in (0, 1):   # open winners in both halves of a group
            assert bool((cols[:, :, h::2] < CHUNK).any())
    if ns == 16:
        for lgi in (0, 1):  # open winners in both groups of a chunk
            assert set(cols[:, lgi].unique().tolist()) == set(range(16 * lgi, 16 * lgi + 16)) | {CHUNK}
    per = split(T, LEAST)[1]
    at = torch.arange(T, device=cols.device)
    meet = {}
    for step in (1, 2):
        same = (cols[:, :, step:] == cols[:, :, :-step]) & (cols[:, :, step:] < CHUNK)
        one_range = (at[step:] // per) == (at[:-step] // per)
        meet[step] = int((same & one_range.view(1, 1, -1)).sum())
        assert meet[step] > 0, "no thread writes one column in the chunks c and c + %d" % step
    shut = 1.0 - open_.double().mean().item()
    assert MIN_SHARE < shut < 1 - MIN_SHARE, shut
    return {"shut": shut, "gate2_slack": slack, "gate3_margin": margin, "meet": meet}


# ------------------------------------------------------------------ truth and yardstick
def reference64(inp, fwd):
    """-> dict of float64 tensors: dq (b,64,r), dw (128,64), s_xhat = sum(gate dq xhat2), s_one =
    sum(gate dq) per channel of layer 2, coef0 = gamma2 invstd2.  The reference module's layer (conv
    1x1, no bias; BatchNorm2d on batch statistics; ReLU; max over nsample -- pytorch_utils.py:14-39,
    70-124, pointnet2_modules.py:256-262) on a2 = relu(bn2(y2)) as a leaf, gathered at the given
    winners.  With fwd["sparse_only"] the statistics are constants, as in an eval-mode BatchNorm: the
    gradient is then W3^T S and S a2^T."""
    b, m, ns, r = inp["b"], inp["m"], inp["ns"], inp["r"]
    y2 = inp["y2"].double().view(b, K_IN, r)
    z2 = y2 * _col(fwd["sc2"]) + _col(fwd["sh2"])
    a2 = torch.relu(z2).requires_grad_(True)
    w3 = inp["w3"].double().requires_grad_(True)
    y3 = torch.einsum("ok,bkr->bor", w3, a2)
    mean = y3.mean(dim=(0, 2), keepdim=True)
    var = y3.var(dim=(0, 2), unbiased=False, keepdim=True)
    if fwd["sparse_only"]:
        mean, var = mean.detach(), var.detach()
    act = torch.relu((y3 - mean) / torch.sqrt(var + EPS) * _col(inp["g3"]) + _col(inp["be3"]))
    at = torch.gather(act.view(b, M_OUT, m, ns), 3, fwd["argmax"].long().unsqueeze(-1)).squeeze(-1)
    (at * inp["dpooled"].double()).sum().backward()
    dq = a2.grad
    gated = torch.where(z2 > 0, dq, torch.zeros((), dtype=torch.float64, device=dq.device))
    xhat2 = (y2 - _col(fwd["mean2"])) * _col(fwd["invstd2"])
    return {"dq": dq, "dw": w3.grad, "s_xhat": (gated * xhat2).sum(dim=(0, 2)), "s_one": gated.sum(dim=(0, 2)),
            "coef0": inp["g2"].double() * fwd["invstd2"].double()}


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


def plain_fp32(inp, fwd):
    """The same five outputs from fp32 torch ops on the same fp32 inputs: a2 = relu(y2 sc2 + sh2),
    y3 = W3 a2, dy3 = a (g - c1 - xhat3 c2) with g the pooled gradient at the winners whose gate
    ymax sc3 + sh3 is open, dq = W3^T dy3, dw = dy3 a2^T, the sums over the gated dq."""
    b, m, ns, r = inp["b"], inp["m"], inp["ns"], inp["r"]
    with _tf32_off():
        y2 = inp["y2"].view(b, K_IN, r)
        z2 = y2 * _c32(fwd["sc2"]) + _c32(fwd["sh2"])
        a2 = torch.relu(z2)
        y3 = torch.matmul(inp["w3"], a2)
        open_ = (fwd["ymax"] * _c32(fwd["sc3"]) + _c32(fwd["sh3"])) > 0
        gsel = torch.where(open_, inp["dpooled"], torch.zeros((), device=y2.device))
        g = torch.zeros(b, M_OUT, m, ns, device=y2.device)
        g.scatter_(3, fwd["argmax"].long().unsqueeze(-1), gsel.unsqueeze(-1))
        coef = fwd["coef3"]
        xhat3 = (y3 - _c32(fwd["mean3"])) * _c32(fwd["invstd3"])
        dy3 = _c32(coef[:, 0].contiguous()) * (g.view(b, M_OUT, r) - _c32(coef[:, 1].contiguous())
                                               - xhat3 * _c32(coef[:, 2].contiguous()))
        del xhat3, g, y3
        dq = torch.matmul(inp["w3"].t(), dy3)
        dw = torch.matmul(dy3, a2.transpose(1, 2)).sum(dim=0)
        gated = torch.where(z2 > 0, dq, torch.zeros((), device=y2.device))
        xhat2 = (y2 - _c32(fwd["mean2"])) * _c32(fwd["invstd2"])
        return {"dq": dq, "dw": dw, "s_xhat": (gated * xhat2).sum(dim=(0, 2)), "s_one": gated.sum(dim=(0, 2)),
                "coef0": inp["g2"] * fwd["invstd2"]}


def sums_resolution(inp, fwd, ref):
    """What ONE fp32 ulp on every element of dq is worth in the two sums, in the two measures of
    errors(): F[k] = ULP * sum over the gated columns of |dq| (times |xhat2| for s_xhat), from the float64
    dq (pool_gram256_cases.sums_resolution says why the sums get this floor).
    -> {"s_one": (||F|| / ||s_one||, max F / max |s_one|), "s_xhat": ...}"""
    b, r = inp["b"], inp["r"]
    y2 = inp["y2"].double().view(b, K_IN, r)
    gate = (y2 * _col(fwd["sc2"]) + _col(fwd["sh2"])) > 0
    mag = torch.where(gate, ref["dq"].abs(), torch.zeros((), dtype=torch.float64, device=y2.device))
    xhat2 = ((y2 - _col(fwd["mean2"])) * _col(fwd["invstd2"])).abs()
    out = {}
    for name, f in (("s_one", ULP * mag.sum(dim=(0, 2))), ("s_xhat", ULP * (mag * xhat2).sum(dim=(0, 2)))):
        out[name] = ((f.norm() / ref[name].norm()).item(), (f.max() / ref[name].abs().max()).item())
    return out


def within(name, e, e32, resolution=None):
    """The rule of the GPU test for one output: both measures of e (errors() of the kernel against
    float64) at most RATIO times plain fp32's e32 plus the floors the number format gives -- one fp32 ulp
    of the range on the max measure, sums_resolution on the two sums.  -> (ok, bound)"""
    own = (resolution or {}).get(name, (0.0, 0.0))
    bound = bound_of(e32, (own[0], own[1] + ULP))
    return e[0] <= bound[0] and e[1] <= bound[1], bound


# ------------------------------------------------------------------ the kernel's algebra, term by term
HI, MID, LO = 0, 1, 2
# the partial products mfma_x6 keeps of the nine, (term of the first operand, term of the second)
SIX = ((LO, HI), (HI, LO), (MID, MID), (MID, HI), (HI, MID), (HI, HI))


def _terms(x, terms):
    """x (fp32 values) -> its three bf16 terms as float64 arrays (mlp_frag.h: split_terms), those from
    `terms` on zero"""
    import numpy as np
    out = [bf16_terms(x, 1)]
    out.append(bf16_terms(x, 2) - out[0])
    out.append(np.ascontiguousarray(x, dtype=np.float32).astype(np.float64) - out[0] - out[1])
    return [t if i < terms else np.zeros_like(t) for i, t in enumerate(out)]


def gram_form64(inp, fwd, terms=3, products=SIX, s_terms=None):
    """The pass's own formulas in float64 numpy -- dq = M3 a2 + v + W3^T S, dw = diag(q) W3 (a2 a2^T) +
    p (sum a2)^T + S a2^T -- as the kernel forms them: q, p, M3, v and a dpooled rounded to fp32, every
    operand of the four matrix products (M3, a2, W3, S) cut to its first `terms` bf16 terms (S to s_terms
    where given) and only the listed partial products (term of the first operand, term of the second)
    summed.  -> dict(dq, dw).  Small rows only (S is dense)."""
    import numpy as np
    b, m, ns, r = inp["b"], inp["m"], inp["ns"], inp["r"]
    f64 = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    coef, mean3, inv3, w = f64(fwd["coef3"]), f64(fwd["mean3"]), f64(fwd["invstd3"]), f64(inp["w3"])
    a, c1, c2 = coef[:, 0], coef[:, 1], coef[:, 2]
    q = f32(-(a * f32(inv3 * c2)))
    p = f32(a * f32(f32(inv3 * c2) * mean3 - c1))
    m3 = f32((w.T * q) @ w)
    v = f32(w.T @ p)
    y2 = f64(inp["y2"]).reshape(b, K_IN, r)
    a2 = f32(np.maximum(y2 * f64(fwd["sc2"])[None, :, None] + f64(fwd["sh2"])[None, :, None], 0.0))
    open_ = (f64(fwd["ymax"]) * f64(fwd["sc3"])[None, :, None] + f64(fwd["sh3"])[None, :, None]) > 0
    val = (fwd["coef3"][:, 0].view(1, -1, 1) * inp["dpooled"]).detach().cpu().double().numpy()   # fp32 a * dpooled
    s = np.zeros((b, M_OUT, m, ns))
    np.put_along_axis(s, fwd["argmax"].detach().cpu().numpy().astype(np.int64)[..., None],
                      np.where(open_, val, 0.0)[..., None], axis=3)
    s = s.reshape(b, M_OUT, r)
    m3_t, w_t, a2_t = _terms(m3, terms), _terms(w, terms), _terms(a2, terms)
    s_t = _terms(s, terms if s_terms is None else s_terms)

    def product(spec, first, second):
        return sum(np.einsum(spec, first[i], second[j]) for i, j in products)

    dq = product("kj,bjr->bkr", m3_t, a2_t) + v[None, :, None] + product("ok,bor->bkr", w_t, s_t)
    gram = product("bkr,bjr->kj", a2_t, a2_t)
    dw = (q[:, None] * w) @ gram + np.outer(p, a2.sum(axis=(0, 2))) + product("bor,bkr->ok", s_t, a2_t)
    return {"dq": dq, "dw": dw}
