"""Inputs, float64 truth and the shape list for the tests of the one-pass eval MLP kernels
(csrc/mlp_eval_pool.hip: eval_lin4_kernel<NS>, eval_stored_kernel<NS, M2B>); no package import.

  weights(form, c_out, seed)   seeded fp32 weights and folded (scale, shift) pairs, built directly (no
                      module, no folding step: what is measured is the kernel, not fold_bn):
                      "lin4":   w0 (64,4), w1 (64,64), w2 (128,64), coeff0 (64), coeff1 (64), coeff2 (128)
                      "stored": w1 (128,128), w2 (c_out,128), coeff0 (128: applied to the stored y0),
                                coeff1 (128), coeff2 (c_out)
                      About 20 % of every scale vector is negative.  The channels BIG_CH of the FIRST
                      affine cancel a mean of 40 (shift0 = -40 scale0 w + O(0.2)); the inputs below
                      carry that mean.  The output channels NEG_CH have shift2 = -50: bn(y) < 0 for every
                      sample of every group, so the pooled output there is exactly 0.
  input_stored(b, m, ns, seed)  y0 (b,128,m,ns): randn, the channels BIG_CH at randn * 2 + 40.
  input_lin4(b, m, ns, seed)    x4 (b,4,m,ns): randn, channel 3 at randn * 2 + 40 (w0[:, 3] is small
                      outside BIG_CH_LIN4, so only those layer-0 channels see the large mean).
  truth_lin4 / truth_stored     the operation with the fp32 operands promoted to float64 ->
                      (pooled output, group maximum before the ReLU).
  plain_fp32(form, x, wts)      the same in fp32 torch ops (einsum, TF32 off): the yardstick any fp32
                      evaluation is held against.
  rel_err(v, truth)             max |v - truth| / max |truth|.
  STORED_SHAPES / LIN4_SHAPES   every tested launch with its tile arithmetic spelled out;
                      tile_arith(...) is the formula tests/test_eval_pool_cases.py checks them with.

A tile is 32 consecutive columns (samples) of one cloud; a wave owns `tpw` consecutive tiles and a
workgroup four waves, so a workgroup holds 4 * tpw consecutive tiles of the flat (cloud, tile) order.
The STORED launch takes tpw = 2 for ns 64 and where the chip is covered anyway; which of the two a
shape gets is the library's decision (mlp_eval_stored_tiles_per_wave), asserted by the GPU test, and
the T of the "c" shapes is found by asking it.  The LIN4 launch always has tpw = 2 and its gate
(m * ns % 256 == 0) makes every cloud a whole number of workgroups: that form has no partial
workgroup and no workgroup that spans two clouds.
"""
import contextlib

import torch

BIG_CH = (3, 50, 77, 127)        # stored y0 channels with mean 40 (both half-waves, first and last k step)
BIG_CH_LIN4 = (3, 21, 40, 62)    # layer-0 channels of the lin4 form whose w0[:, 3] is not damped
NEG_CH = {128: (5,), 256: (5, 200)}   # output channels that no sample makes positive (both halves of 256)
BIG_MEAN = 40.0
# e(kernel) <= RATIO * e(plain_fp32), both against float64 on the same data (tests/test_gpu_mlp.py
# _grad_bound's margin; DESIGN.md, inference section, has the measured figures)
RATIO = 3

# ---- the shape lists.  STORED: (case, ns, b, m, tpw, tiles_per_cloud, total_tiles, workgroups,
# live tiles of the last workgroup); every one runs at C_out 128 and 256.  m = None ("c"): m = T * 32 / ns
# with T found on the device; the arithmetic listed is that of T = 1367, what a 256-CU chip gives.
STORED_SHAPES = (
    # (a) one cloud, less than one workgroup
    ("a", 16, 1, 6, 1, 3, 3, 1, 3),
    ("a", 32, 1, 3, 1, 3, 3, 1, 3),
    ("a", 64, 1, 3, 2, 6, 6, 1, 6),          # waves 0-2 hold a group each, wave 3 idle
    # (b) three such clouds: workgroup 0 holds tiles of clouds 0 and 1, the last one tile / one wave
    ("b", 16, 3, 6, 1, 3, 9, 3, 1),
    ("b", 32, 3, 3, 1, 3, 9, 3, 1),
    ("b", 64, 3, 3, 2, 6, 18, 3, 2),
    # (c) two tiles per wave with a tail; T odd: a wave's pair straddles the cloud boundary
    ("c", 16, 3, None, 2, 1367, 4101, 513, 5),
    ("c", 32, 3, None, 2, 1367, 4101, 513, 5),
    # (d) aligned
    ("d", 16, 2, 256, 1, 128, 256, 64, 4),
    ("d", 32, 2, 256, 1, 256, 512, 128, 4),
    ("d", 64, 2, 256, 2, 512, 1024, 128, 8),
)
TAIL_CASES = ("a", "b", "c")        # total_tiles % (4 * tpw) != 0
BOUNDARY_CASES = ("b", "c")         # tiles_per_cloud % 4 != 0: some workgroup holds two clouds' tiles
C_START_T = 129                     # the upward search for T starts here (odd; far below any chip's answer)

# LIN4: (case, ns, b, m, tiles_per_cloud, total_tiles, workgroups); tpw = 2, eight tiles per workgroup
LIN4_SHAPES = (
    ("one_wg", 16, 1, 16, 8, 8, 1), ("one_wg", 32, 1, 8, 8, 8, 1), ("one_wg", 64, 1, 4, 8, 8, 1),
    ("one_wg_b3", 16, 3, 16, 8, 24, 3), ("one_wg_b3", 32, 3, 8, 8, 24, 3), ("one_wg_b3", 64, 3, 4, 8, 24, 3),
    ("three_wg", 16, 2, 48, 24, 48, 6), ("three_wg", 32, 2, 24, 24, 48, 6), ("three_wg", 64, 2, 12, 24, 48, 6),
    ("m2048", 16, 1, 2048, 1024, 1024, 128), ("m2048", 32, 1, 2048, 2048, 2048, 256),
    ("m2048", 64, 1, 2048, 4096, 4096, 512),
)


def tile_arith(b, m, ns, tpw):
    """-> (tiles_per_cloud, total_tiles, workgroups, live tiles of the last workgroup)"""
    r = m * ns
    assert r % 32 == 0
    tpc = r // 32
    total = b * tpc
    per_wg = 4 * tpw
    wgs = -(-total // per_wg)
    return tpc, total, wgs, total - (wgs - 1) * per_wg


def stored_gate(b, c_out, m, ns):
    """mlp_eval_stored_supported's formula"""
    return b > 0 and m > 0 and c_out in (128, 256) and ns in (16, 32, 64) and (m * ns) % 32 == 0


def lin4_gate(b, m, ns):
    """mlp_eval_lin4_supported's formula"""
    return b > 0 and m > 0 and ns in (16, 32, 64) and (m * ns) % 256 == 0


def m_of_tiles(t, ns):
    """the m whose cloud has t tiles"""
    assert (t * 32) % ns == 0
    return t * 32 // ns


def find_c_tiles(tiles_per_wave, c_out, ns, b=3, limit=1 << 16):
    """Smallest odd T >= C_START_T with tiles_per_wave(b, c_out, m(T), ns) == 2 and b * T % 8 != 0, by
    asking the library (tiles_per_wave is its exported query), never from a CU count."""
    t = C_START_T
    while t < limit:
        if tiles_per_wave(b, c_out, m_of_tiles(t, ns), ns) == 2 and (b * t) % 8 != 0:
            return t
        t += 2
    raise AssertionError("no two-tiles-per-wave shape below %d tiles per cloud" % limit)


# ------------------------------------------------------------------ builders
def _scale_shift(c, g):
    sign = torch.where(torch.rand(c, generator=g) < 0.2, -1.0, 1.0)
    return (sign * (0.5 + torch.rand(c, generator=g))).float(), (torch.randn(c, generator=g) * 0.2).float()


def weights(form, c_out=128, seed=0, device="cpu"):
    """-> dict(form, w: tuple of fp32 weights, coeff: tuple of (scale, shift) fp32 pairs); see the header"""
    g = torch.Generator().manual_seed(1000 * seed + c_out + (7 if form == "lin4" else 0))
    if form == "lin4":
        assert c_out == 128
        w0 = torch.randn(64, 4, generator=g) * 0.5
        damp = torch.full((64,), 0.05)
        damp[list(BIG_CH_LIN4)] = 1.0
        w0[:, 3] *= damp
        w1 = torch.randn(64, 64, generator=g) * (2.0 / 64) ** 0.5
        w2 = torch.randn(128, 64, generator=g) * (2.0 / 64) ** 0.5
        c0, c1, c2 = _scale_shift(64, g), _scale_shift(64, g), _scale_shift(128, g)
        # every layer-0 channel's mean is 40 w0[:, 3]; the affine takes it out, as a BatchNorm would
        sh0 = (c0[1].double() - c0[0].double() * BIG_MEAN * w0[:, 3].double()).float()
        c0 = (c0[0], sh0)
        ws = (w0, w1, w2)
    else:
        assert form == "stored" and c_out in (128, 256)
        w1 = torch.randn(128, 128, generator=g) * (2.0 / 128) ** 0.5
        w2 = torch.randn(c_out, 128, generator=g) * (2.0 / 128) ** 0.5
        c0, c1, c2 = _scale_shift(128, g), _scale_shift(128, g), _scale_shift(c_out, g)
        sh0 = c0[1].clone()
        big = list(BIG_CH)
        sh0[big] = (c0[1][big].double() - c0[0][big].double() * BIG_MEAN).float()
        c0 = (c0[0], sh0)
        ws = (w1, w2)
    sh2 = c2[1].clone()
    sh2[list(NEG_CH[c_out])] = -50.0
    c2 = (c2[0], sh2)
    dev = torch.device(device)
    return {"form": form, "w": tuple(w.float().contiguous().to(dev) for w in ws),
            "coeff": tuple((s.contiguous().to(dev), h.contiguous().to(dev)) for s, h in (c0, c1, c2))}


def input_stored(b, m, ns, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(77 + seed)
    y0 = torch.randn(b, 128, m, ns, generator=g)
    big = list(BIG_CH)
    y0[:, big] = y0[:, big] * 2 + BIG_MEAN
    return y0.contiguous().to(torch.device(device))


def input_lin4(b, m, ns, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(99 + seed)
    x4 = torch.randn(b, 4, m, ns, generator=g)
    x4[:, 3] = x4[:, 3] * 2 + BIG_MEAN
    return x4.contiguous().to(torch.device(device))


# ------------------------------------------------------------------ the operation
def _layers(form, wts):
    """[(w or None, (scale, shift))]: the stored form starts with an affine on the stored y0"""
    ws, cs = wts["w"], wts["coeff"]
    return list(zip(ws if form == "lin4" else (None,) + tuple(ws), cs))


def _run(form, x, wts, dtype):
    y = x.to(dtype)
    layers = _layers(form, wts)
    for i, (w, (scale, shift)) in enumerate(layers):
        if w is not None:
            y = torch.einsum("ok,bkmn->bomn", w.to(dtype), y)
        y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
        if i + 1 < len(layers):
            y = torch.relu(y)
    pre = y.amax(3)
    return torch.relu(pre), pre


def truth_lin4(x4, wts):
    """x4 (b,4,m,ns) -> (pooled (b,128,m), group maximum before the ReLU), float64"""
    return _run("lin4", x4, wts, torch.float64)


def truth_stored(y0, wts):
    """y0 (b,128,m,ns) -> (pooled (b,C_out,m), group maximum before the ReLU), float64"""
    return _run("stored", y0, wts, torch.float64)


@contextlib.contextmanager
def _tf32_off():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old


def plain_fp32(form, x, wts):
    """the pooled output in fp32 torch ops"""
    with _tf32_off():
        return _run(form, x, wts, torch.float32)[0]


def rel_err(v, truth):
    """e(v) = max |v - truth| / max |truth|"""
    return ((v.double() - truth).abs().max() / truth.abs().max()).item()
