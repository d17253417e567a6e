"""Shapes, inputs, float64 truth and fp32 yardstick for the tests of the 128 -> 256 Gram backward
(csrc/mlp_pool_gram256.hip: prep, pack, dgrad<16|32>, wgrad<16|32>, reduce, dw); no package import.

Both passes are persistent: with T = b * r / 32 chunks of 32 columns, g = max(1, min(CUs, T / least))
workgroups (least = 8 for the data-gradient pass, 16 for the weight-gradient pass) and
per = ceil(T / g), workgroup i owns the chunks [i * per, min(i * per + per, T)).  A range may be empty,
one chunk (the look-ahead re-fetches the chunk itself), odd (the last chunk runs on buffer 0 alone),
even, and may run from one cloud into the next.  The reduce kernel sums the weight pass's g partials
four at a time per slice of eight while p + 24 < g, one at a time after that.

  split(T, least, cus)            (g, per, ranges): gram256_workgroups and the kernels' per / c_lo / c_hi
  describe(b, m, ns, least, cus)  what the ranges of one pass look like for a row of CASES
  workspace_floats(...)           mlp_pool_gram_workspace_floats' formula
  CASES                           (b, groups m, ns, seed); r = m * ns.  tests/test_pool_gram256_cases.py
                                  proves on the CPU that they reach every edge above at 256 CUs; the
                                  GPU test asserts that the device's own counts are the mirror's.
  make_inputs(b, m, ns, seed)     y2 = randn * 1.3 + 0.2 with column 3 a copy of column 1 in every
                                  third group (pool ties: the first index wins; in the other groups
                                  position 3 can win), w3, BatchNorm weights with every fifth channel
                                  negative on both layers, a bias of -2 on every seventh channel of
                                  layer 3 (its pooled ReLU is shut in about half of the groups), dpooled.
  forward64(inp)                  what the backward consumes -- both layers' statistics and folded
                                  (scale, shift), arg-max, ymax, coef3 -- from torch in float64, rounded
                                  to fp32: no kernel of the project prepares the test's inputs.
  check_inputs(inp, fwd)          the conditions on the data, asserted before anything is compared.
  reference64(inp, fwd)           the reference module's layer in float64 with autograd (conv 1x1, no
                                  bias; BatchNorm2d on batch statistics; ReLU; max over nsample --
                                  pytorch_utils.py:14-39,70-124, pointnet2_modules.py:256-262) on
                                  a2 = relu(bn2(y2)) as a leaf, gathered at the given winners.
  plain_fp32(inp, fwd)            the same outputs from plain fp32 torch ops: two matmuls and the
                                  BatchNorm-backward algebra on the same fp32 inputs.
  errors(got, truth)              (relative L2 error, max error over the truth's range)
  sums_resolution(inp, fwd, ref)  what one fp32 ulp per element of dq is worth in the sums over it
  gram_form64(inp, fwd, terms)    the pass's own formulas in float64 numpy, a2 cut to `terms` bf16 terms
"""
import contextlib

import torch

K_IN, M_OUT, CHUNK = 128, 256, 32
DGRAD_LEAST, WGRAD_LEAST = 8, 16
CUS = 256                     # the CU count the table was laid out for
SUMS = K_IN * K_IN + K_IN + M_OUT * K_IN
EPS = 1e-5
RATIO = 3                     # e(kernel) <= RATIO * e(plain fp32), tests/test_gpu_mlp.py::_grad_bound's margin
SHUT_BIAS = -2.0
TWIN_EVERY = 3                # the groups 0, 3, 6, ... carry the twin columns 1 and 3
OUTPUTS = ("dq", "dw", "s_xhat", "s_one", "coef0")

# (b, groups m, ns, seed).  The seeds are those at which check_inputs holds (no ReLU gate of either
# layer within rounding of zero); most seeds do, the large rows need a few tries.
CASES = (
    (1, 1, 32, 1),       # T = 1: one chunk, one group
    (1, 2, 16, 0),       # T = 1: one chunk, two groups
    (1, 3, 32, 0),       # T = 3: one odd range
    (2, 64, 16, 0),      # T = 64: the even split; 64 groups = two whole blocks of the pack kernel
    (3, 27, 32, 0),      # T = 81
    (17, 17, 32, 0),     # T = 289: 15 crossing data ranges, a last data range of one chunk
    (3, 50, 16, 0),      # T = 75
    (2, 330, 16, 0),     # T = 330
    (2, 201, 32, 2),     # T = 402: 25 weight partials
    (5, 129, 32, 0),     # T = 645
    (2, 460, 16, 0),     # T = 460 = 51 * 9 + 1 = 27 * 17 + 1: both passes end in a range of one chunk
    (5, 92, 32, 1),      # T = 460 again, one group per chunk, four cloud boundaries inside ranges
    (1, 4112, 16, 1),    # T = 2056: the data pass at the CU count
    (2, 2056, 32, 6),    # T = 4112: both passes at the CU count
)


# ------------------------------------------------------------------ the split
def covers(b, r, ns):
    """gram256_covers"""
    return b > 0 and r > 0 and r % 32 == 0 and ns in (16, 32) and r % ns == 0


def split(T, least, cus=CUS):
    """-> (g, per, [(c_lo, c_hi)] * g) as gram256_workgroups and the kernels compute them"""
    g = max(1, min(cus, T // least))
    per = (T + g - 1) // g
    return g, per, [(i * per, min(i * per + per, T)) for i in range(g)]


def chunks(b, m, ns):
    return b * (m * ns // CHUNK)


def describe(b, m, ns, least, cus=CUS):
    """-> dict(T, g, per, empty, lengths: set of the non-empty ranges' lengths, crossing: ranges whose
    chunks lie in more than one cloud)"""
    per_cloud = m * ns // CHUNK
    T = b * per_cloud
    g, per, ranges = split(T, least, cus)
    live = [(lo, hi) for lo, hi in ranges if lo < hi]
    return {"T": T, "g": g, "per": per, "empty": len(ranges) - len(live),
            "lengths": {hi - lo for lo, hi in live},
            "crossing": sum(1 for lo, hi in live if lo // per_cloud != (hi - 1) // per_cloud)}


def workspace_floats(b, m, ns, cus=CUS):
    """mlp_pool_gram256_workspace_floats: qp, M3, v, the records, the weight pass's partials, the sums
    as doubles, 16 spare"""
    g2 = split(chunks(b, m, ns), WGRAD_LEAST, cus)[0]
    return 512 + 16384 + 128 + b * m * M_OUT * 2 + g2 * SUMS + 2 * SUMS + 16


def records_offset_floats():
    return 512 + 16384 + 128


def sums_offset_floats(b, m, ns, cus=CUS):
    g2 = split(chunks(b, m, ns), WGRAD_LEAST, cus)[0]
    return records_offset_floats() + b * m * M_OUT * 2 + g2 * SUMS


# ------------------------------------------------------------------ inputs
def make_inputs(b, m, ns, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(100003 * seed + 1009 * b + 10 * m + ns)
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


def forward64(inp):
    """-> dict of fp32 tensors: mean2, invstd2, sc2, sh2, mean3, invstd3, sc3, sh3, argmax (int32), ymax,
    coef3 (256,3) = (gamma invstd, sum g / N, sum g xhat / N) with g the gated pooled gradient"""
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
    open_ = (ymax.double() * _col(sc3) + _col(sh3)) > 0   # the kernels' gate, fmaf(ymax, sc3, sh3) > 0
    gsel = torch.where(open_, inp["dpooled"].double(), torch.zeros((), dtype=torch.float64, device=ymax.device))
    xhat = (ymax.double() - _col(mean3)) * _col(invstd3)
    n = float(b) * float(r)
    coef3 = torch.stack([inp["g3"].double() * invstd3.double(), gsel.sum(dim=(0, 2)) / n,
                         (gsel * xhat).sum(dim=(0, 2)) / n], dim=1).float().contiguous()
    return {"mean2": mean2, "invstd2": invstd2, "sc2": sc2, "sh2": sh2, "mean3": mean3, "invstd3": invstd3,
            "sc3": sc3, "sh3": sh3, "argmax": first.int().contiguous(), "ymax": ymax, "coef3": coef3}


GATE_ULPS = 4                 # layer 2: |z| > GATE_ULPS * eps32 * (|y2 sc2| + |sh2|), z in float64
POOL_MARGIN = 1e-5            # layer 3: |bn3(y3 at the winner)| in float64, against values of order 1
MIN_SHARE = 0.02


def check_inputs(inp, fwd):
    """The conditions on the data (asserted, not excused afterwards) -> dict of the measured shares.
    * No layer-2 pre-activation y2 sc2 + sh2 within GATE_ULPS fp32 roundings of zero: the kernels' fused
      multiply-add has the sign of the exact value, and so does any fp32 evaluation that far from zero.
    * No pooled pre-activation of layer 3 within POOL_MARGIN of zero, in float64 on float64 statistics:
      the kernels decide on fmaf(fp32 ymax, fp32 scale, fp32 shift), some 1e-6 away from that.
    * The winners take every column of a chunk that they can (position 3 of a group with the twin columns
      is the later twin and never wins; the rows with one or two groups lose that column); with ns = 16
      so do the winners whose ReLU is open, in both groups of a chunk.
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
    z3 = (y3 - mean) / torch.sqrt(var + EPS) * _col(inp["g3"]) + _col(inp["be3"])
    am = fwd["argmax"].long()
    zw = torch.gather(z3.view(b, M_OUT, m, ns), 3, am.unsqueeze(-1)).squeeze(-1)
    assert zw.abs().min().item() > POOL_MARGIN, "a pooled ReLU gate within %g of zero: take another seed" % POOL_MARGIN
    open_ = (fwd["ymax"].double() * _col(fwd["sc3"]) + _col(fwd["sh3"])) > 0
    assert bool((open_ == (zw > 0)).all())
    assert float((zw - z3.view(b, M_OUT, m, ns).amax(3)).abs().max()) <= 1e-9   # the winners are the maxima
    assert not bool((am[:, :, ::TWIN_EVERY] == 3).any()), "a later twin won"
    per_chunk = CHUNK // ns   # groups per chunk; a winner's column in its chunk is (group % per_chunk) * ns + position
    possible = {(j % per_chunk) * ns + p for j in range(m) for p in range(ns) if not (j % TWIN_EVERY == 0 and p == 3)}
    col = am + ns * (torch.arange(m, device=am.device) % per_chunk).view(1, 1, m)
    assert set(col.unique().tolist()) == possible
    if ns == 16:
        assert set(col[open_].unique().tolist()) == possible   # open entries in both groups of a chunk
    shut = 1.0 - open_.double().mean().item()
    assert MIN_SHARE < shut < 1 - MIN_SHARE, shut
    return {"shut": shut, "gate2_slack": slack, "gate3_margin": zw.abs().min().item()}


# ------------------------------------------------------------------ truth and yardstick
def reference64(inp, fwd):
    """-> dict of float64 tensors: dq (b,128,r), dw (256,128), s_xhat = sum(gate dq xhat2), s_one =
    sum(gate dq) per channel of layer 2, coef0 = gamma2 invstd2"""
    b, m, ns, r = inp["b"], inp["m"], inp["ns"], inp["r"]
    y2 = inp["y2"].double().view(b, K_IN, r)
    z2 = y2 * _col(fwd["sc2"]) + _col(fwd["sh2"])
    a2 = torch.relu(z2).requires_grad_(True)
    w3 = inp["w3"].double().requires_grad_(True)
    y3 = torch.einsum("ok,bkr->bor", w3, a2)
    mean = y3.mean(dim=(0, 2), keepdim=True)
    var = y3.var(dim=(0, 2), unbiased=False, keepdim=True)
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


def errors(got, truth):
    """-> (||got - truth|| / ||truth||, max |got - truth| / max |truth|)"""
    d = got.double().reshape(truth.shape) - truth
    return (d.norm() / truth.norm()).item(), (d.abs().max() / truth.abs().max()).item()


ULP = 2.0 ** -23              # one fp32 ulp of a value, relative to it, at most


def bound_of(e32, floor=(0.0, 0.0)):
    """what the kernel may err by: RATIO times the fp32 yardstick's own error, per measure, plus a floor"""
    return tuple(RATIO * e + f for e, f in zip(e32, floor))


def sums_resolution(inp, fwd, ref):
    """What ONE fp32 ulp on every element of dq is worth in the two sums, in the two measures of
    errors(): F[k] = ULP * sum over the gated columns of |dq| (times |xhat2| for s_xhat), from the float64
    dq.  The sums are sums over the pass's own fp32 dq; an error of dq that has one sign in every column
    goes into them whole, however small it is element by element, and the sums of a BatchNorm backward
    cancel to a small part of sum |dq|.  -> {"s_one": (||F|| / ||s_one||, max F / max |s_one|), "s_xhat": ...}"""
    b, r = inp["b"], inp["r"]
    y2 = inp["y2"].double().view(b, K_IN, r)
    gate = (y2 * _col(fwd["sc2"]) + _col(fwd["sh2"])) > 0
    mag = torch.where(gate, ref["dq"].abs(), torch.zeros((), dtype=torch.float64, device=y2.device))
    xhat2 = ((y2 - _col(fwd["mean2"])) * _col(fwd["invstd2"])).abs()
    out = {}
    for name, f in (("s_one", ULP * mag.sum(dim=(0, 2))), ("s_xhat", ULP * (mag * xhat2).sum(dim=(0, 2)))):
        out[name] = ((f.norm() / ref[name].norm()).item(), (f.max() / ref[name].abs().max()).item())
    return out


# ------------------------------------------------------------------ the kernel's algebra, term by term
def bf16_terms(x, terms):
    """x (numpy array of fp32 values, any float type) as the float64 sum of its first `terms` bf16
    terms, each the truncation of what is left (csrc/mlp_pool_gram256.hip: split_terms); three terms
    are the value itself"""
    import numpy as np
    left = np.ascontiguousarray(x, dtype=np.float32)
    total = np.zeros(left.shape, dtype=np.float64)
    for _ in range(terms):
        t = (left.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
        total += t
        left = left - t   # (exact: the difference fits the format)
    return total


def gram_form64(inp, fwd, terms=3):
    """The pass's own formulas in float64 numpy -- dq = M3 a2 + v + W3^T S, dw = diag(q) W3 (a2 a2^T) +
    p (sum a2)^T + S a2^T -- with a2 cut to its first `terms` bf16 terms wherever the kernels read its
    images (M3 a2, the Gram matrix, S a2^T).  -> dict(dq, dw, m3a2, gram, and the same two from exact a2
    and from fp32 matmuls: m3a2_exact, gram_exact, m3a2_fp32, gram_fp32).  Small rows only (S is dense)."""
    import numpy as np
    b, m, ns, r = inp["b"], inp["m"], inp["ns"], inp["r"]
    f64 = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
    coef, mean3, inv3, w = f64(fwd["coef3"]), f64(fwd["mean3"]), f64(fwd["invstd3"]), f64(inp["w3"])
    a, c1, c2 = coef[:, 0], coef[:, 1], coef[:, 2]
    q = -(a * inv3 * c2)
    p = a * (inv3 * c2 * mean3 - c1)
    m3 = ((w.T * q) @ w).astype(np.float32).astype(np.float64)   # (the prep kernel rounds M3 to fp32)
    v = w.T @ p
    y2 = f64(inp["y2"]).reshape(b, K_IN, r)
    a2 = np.maximum(y2 * f64(fwd["sc2"])[None, :, None] + f64(fwd["sh2"])[None, :, None], 0.0)
    a2 = a2.astype(np.float32).astype(np.float64)   # the fused multiply-add's one rounding
    a2t = bf16_terms(a2, terms)
    open_ = (f64(fwd["ymax"]) * f64(fwd["sc3"])[None, :, None] + f64(fwd["sh3"])[None, :, None]) > 0
    val = (fwd["coef3"][:, 0].view(1, -1, 1) * inp["dpooled"]).detach().cpu().double().numpy()   # fp32 a * dpooled
    s = np.zeros((b, M_OUT, m, ns))
    np.put_along_axis(s, fwd["argmax"].detach().cpu().numpy().astype(np.int64)[..., None],
                      np.where(open_, val, 0.0)[..., None], axis=3)
    s = s.reshape(b, M_OUT, r)
    m3a2, gram = m3 @ a2t, np.einsum("bkr,bjr->kj", a2t, a2t)
    dq = m3a2 + v[None, :, None] + np.einsum("ok,bor->bkr", w, s)
    dw = (q[:, None] * w) @ gram + np.outer(p, a2.sum(axis=(0, 2))) + np.einsum("bor,bkr->ok", s, a2t)
    m3_32, a2_32 = m3.astype(np.float32), a2.astype(np.float32)
    return {"dq": dq, "dw": dw, "m3a2": m3a2, "gram": gram,
            "m3a2_exact": m3 @ a2, "gram_exact": np.einsum("bkr,bjr->kj", a2, a2),
            "m3a2_fp32": np.matmul(m3_32, a2_32), "gram_fp32": np.einsum("bkr,bjr->kj", a2_32, a2_32)}
