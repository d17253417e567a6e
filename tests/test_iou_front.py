"""The IoU branch's fused front end (csrc/gridconv_front.hip: bbox_jitter_kernel, gridconv_points_kernel,
three_nn_weights_kernel) against the formulas it replaces.

  1. one seeded builder of EDGE inputs (negative / zero / -0.0 decoded sizes, the 1e-8 clamp of the
     jittered size, headings at float32(pi), one ulp above it and still above pi after the wrap, the
     winning class in the first and in the last position, a tie set);
  2. each kernel against the fp32 tensor formulation that sits beside it in the package, on the same
     device and the same inputs, BIT FOR BIT.  Two operations could round differently from the tensor
     library's; each has an isolated test.  Measured on the MI355X (ROCm 7 torch): the device sinf / cosf
     ARE torch.sin / cos bit for bit, so the grid stays under bit equality; the library's sum over the
     three neighbours is NOT the kernel's (w0 + w1) + w2 -- it adds (w0 + w2) + w1 -- so the normalised
     weights, and only they, are bit-equal where the order cannot matter and within the float64 bound of
     part 3 elsewhere, and bit-equal everywhere to the IEEE fp32 evaluation of the documented order;
  3. each kernel against a float64 evaluation on the CPU, with bounds that count roundings;
  4. the REFERENCE's own VoteNet.forward_with_pred_jitter + GridConv.forward at the same edges
     (tests/golden/iou_front_ref.npz, made by tests/golden/make_iou_front_golden.py): CPU leg through
     this package's tensor path, GPU leg through the kernels;
  5. the paths of the module (fused / PN2_INTERP_FIRST=0 / the recording path of evaluate_with_opt)
     against each other and a float64 truth;
  6. the argument checks of the three entry points (rejected on the host, nothing launched).

Bit equality is checked on the int32 view of the floats, so 0.0 and -0.0 differ and NaN == NaN.
"""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import golden, load_pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

F32 = np.float32
EPS = 2.0 ** -24  # half an ulp of 1.0: the relative error of ONE fp32 rounding
PI32, TWO_PI32 = F32(np.pi), F32(2 * np.pi)
JITTER32, CLAMP32, TINY32 = F32(0.3), F32(1e-8), F32(1e-6)
# (ns, nh) = size clusters, heading bins: ScanNet, SUN RGB-D and the smallest legal pair
CONFIGS = {"scannet": (18, 1), "sunrgbd": (10, 12), "tiny": (1, 2)}
NUM_CLASS = {"scannet": 18, "sunrgbd": 10, "tiny": 1}
HEAD_SHAPES = [(1, 1), (3, 70), (8, 256)]
GOLDEN_SHAPE = (3, 70)
GOLDEN_SEEDS, GOLDEN_CHANNELS = 64, 16
GRID_SHAPES = [(1, 1), (1, 3), (3, 37), (8, 512)]  # b*k*64 is / is not a multiple of 256
SENTINEL = -12345.678


# ------------------------------------------------------------------ 1. shared edge inputs
def mean_size_table(ns):
    """(ns, 3) seeded mean sizes.  The z entry of the LAST class is -0.0: a decoded size of -0.0 can
    only come from (-0.0 + -0.0) / 2 (round-to-nearest gives x + (-x) == +0.0)."""
    table = np.random.default_rng(100 + ns).uniform(0.3, 1.8, (ns, 3)).astype(F32)
    table[ns - 1, 2] = F32(-0.0)
    return table


def plant_position(p, total):
    """planted proposal number p -> flat proposal index: alternately from the front and from the back
    (the back ones sit in the last, partial workgroup of the kernel), None if the shape is too small"""
    if p >= total:
        return None
    return p // 2 if p % 2 == 0 else total - 1 - p // 2


SIZE_PLANTS = ("size_neg_zero_negzero", "size_first_class", "noise_at_clamp", "noise_below_clamp",
               "noise_center_zero")
HEADING_PLANTS = ("heading_pi", "heading_pi_plus_ulp", "heading_last_wraps", "heading_last_stays_above",
                  "heading_first_negative")


def plant_positions(nh, total):
    names = SIZE_PLANTS + (HEADING_PLANTS if nh > 1 else ())
    out = {}
    for p, name in enumerate(names):
        t = plant_position(p, total)
        if t is not None:
            out[name] = t
    return out


def plant_noise(noise_c, noise_s, plants):
    """the planted draws, written into two (b, k, 3) float32 noise arrays in place"""
    nc, ns_ = noise_c.reshape(-1, 3), noise_s.reshape(-1, 3)
    if "noise_at_clamp" in plants:      # size + size * n * 0.3 lands on / next to 0: clamp to 1e-8
        ns_[plants["noise_at_clamp"]] = F32(-1) / JITTER32
    if "noise_below_clamp" in plants:   # ... clearly below 0
        ns_[plants["noise_below_clamp"]] = (F32(-4.0), np.nextafter(F32(-1) / JITTER32, F32(-10)), F32(-3.5))
    if "noise_center_zero" in plants:
        nc[plants["noise_center_zero"]] = (F32(0.0), F32(-0.0), F32(0.0))


def head_inputs(tag, b, k, seed=0):
    """Seeded head outputs + jitter noise of b x k proposals with the planted edge proposals.
    Returns float32 arrays center (b,k,3), size_scores (b,k,ns), size_residuals (b,k,ns,3),
    heading_scores / heading_residuals (b,k,nh), noise_c / noise_s (b,k,3), mean_size (ns,3) and
    `plants`: name -> flat proposal index."""
    ns, nh = CONFIGS[tag]
    g = np.random.default_rng([seed, ns, nh, b, k])
    total = b * k
    mean = mean_size_table(ns)
    inp = {
        "center": g.uniform(-4, 4, (b, k, 3)).astype(F32),
        "size_scores": g.standard_normal((b, k, ns)).astype(F32),
        "size_residuals": g.uniform(-0.25, 0.5, (b, k, ns, 3)).astype(F32),
        "heading_scores": g.standard_normal((b, k, nh)).astype(F32),
        "heading_residuals": g.uniform(-np.pi / nh, np.pi / nh, (b, k, nh)).astype(F32),
        "noise_c": g.standard_normal((b, k, 3)).astype(F32),
        "noise_s": g.standard_normal((b, k, 3)).astype(F32),
        "mean_size": mean,
    }
    plants = plant_positions(nh, total)
    ss, sr = inp["size_scores"].reshape(total, ns), inp["size_residuals"].reshape(total, ns, 3)
    hs, hr = inp["heading_scores"].reshape(total, nh), inp["heading_residuals"].reshape(total, nh)

    def win(rows, t, cls):
        rows[t, cls] = F32(10.0)  # the other scores are standard normal draws

    if "size_neg_zero_negzero" in plants:  # winning class LAST; sizes < 0, == 0.0, == -0.0 per axis
        t = plants["size_neg_zero_negzero"]
        win(ss, t, ns - 1)
        sr[t, ns - 1] = (-mean[ns - 1, 0] - F32(0.5), -mean[ns - 1, 1], F32(-0.0))
    if "size_first_class" in plants:       # winning class FIRST
        win(ss, plants["size_first_class"], 0)
    plant_noise(inp["noise_c"], inp["noise_s"], plants)
    half = nh // 2                          # half * float32(2 pi / nh) == float32(pi) for nh = 2, 12
    for name, cls, res in (("heading_pi", half, F32(0.0)),
                           ("heading_pi_plus_ulp", half, np.spacing(PI32)),
                           ("heading_last_wraps", nh - 1, F32(0.3)),
                           ("heading_last_stays_above", nh - 1, F32(4.0 if nh > 2 else 7.0)),  # > 3 pi
                           ("heading_first_negative", 0, F32(-0.2))):
        if name in plants:
            win(hs, plants[name], cls)
            hr[plants[name], cls] = res
    inp["plants"] = plants
    return inp


def tie_rows(n):
    """(rows, n) float32 score rows whose maximum is not unique or sits next to -inf entries"""
    ninf = F32(-np.inf)
    rows = [np.full(n, 0.5, F32), np.full(n, ninf, F32)]
    if n >= 2:
        a, c = (1 if n > 2 else 0), n - 1
        two = np.linspace(-1, 0, n).astype(F32); two[a] = two[c] = 2.0        # two equal maxima
        rows.append(two)
        sign = np.full(n, -1, F32); sign[a], sign[c] = -0.0, 0.0                # -0.0 == 0.0: the first
        rows.append(sign)
        sign2 = np.full(n, -1, F32); sign2[a], sign2[c] = 0.0, -0.0
        rows.append(sign2)
        lead = np.linspace(0, 1, n).astype(F32); lead[0] = ninf                 # -inf in front of the max
        rows.append(lead)
        only_last = np.full(n, ninf, F32); only_last[c] = -3.0                  # all -inf but the last
        rows.append(only_last)
        tail = np.linspace(1, 0, n).astype(F32); tail[c] = ninf; tail[0] = tail[a] = 1.0
        rows.append(tail)
    return np.stack(rows)


def grid_boxes(b, k, seed=0, sane=False):
    """centre (b,k,3), HALF size (b,k,3), heading (b,k) for the grid kernel: headings 0, +-float32(pi),
    +-float32(pi/2), +-7 (range reduction) and random in (-pi, pi]; half sizes log-uniform from 1e-8 to
    3 with the two clamp values 1e-8 and 1e-6 planted; centres up to +-50.  sane=True: boxes a detector
    could predict inside a +-4 m scene (sizes 0.05 .. 1.5)."""
    g = np.random.default_rng([seed, b, k, int(sane)])
    total = b * k
    heading = (-g.uniform(-np.pi, np.pi, total)).astype(F32)  # (-pi, pi]
    special = (F32(0.0), PI32, -PI32, F32(np.pi / 2), -F32(np.pi / 2), F32(7.0), F32(-7.0), F32(-0.0))
    for p, h in enumerate(special):
        t = plant_position(p, total)
        if t is not None:
            heading[t] = h
    if sane:
        size = g.uniform(0.05, 1.5, (total, 3)).astype(F32)
        center = g.uniform(-3.5, 3.5, (total, 3)).astype(F32)
    else:
        size = np.exp(g.uniform(np.log(1e-8), np.log(3.0), (total, 3))).astype(F32)
        center = g.uniform(-50, 50, (total, 3)).astype(F32)
        for p, s in enumerate(((CLAMP32, TINY32, F32(3.0)), (F32(3.0), CLAMP32, TINY32), (TINY32,) * 3)):
            t = plant_position(p + 1, total)
            if t is not None:
                size[t] = s
        center[0] = (F32(50.0), F32(-50.0), F32(0.0))
    return center.reshape(b, k, 3), size.reshape(b, k, 3), heading.reshape(b, k)


def seed_cloud(b, m, c, seed=0):
    g = np.random.default_rng([seed, b, m, c])
    return g.uniform(-4, 4, (b, m, 3)).astype(F32), g.standard_normal((b, c, m)).astype(F32)


def nn_clouds(b, n, m, seed=0):
    """unknown (b,n,3), known (b,m,3): query (0, 0) sits ON known point 5 % m (one distance 0); known
    points 7 % m and 8 % m of the last cloud coincide and query (b-1, n-1) sits on them (two distances
    0, where m >= 3); one query of cloud 0 has three EQUAL distances (m >= 9, n >= 3)"""
    g = np.random.default_rng([seed, b, n, m])
    known = g.uniform(-4, 4, (b, m, 3)).astype(F32)
    unknown = g.uniform(-4, 4, (b, n, 3)).astype(F32)
    if m >= 3:
        known[b - 1, 8 % m] = known[b - 1, 7 % m]
        unknown[b - 1, n - 1] = known[b - 1, 7 % m]
    if (b - 1, n - 1) != (0, 0) or m < 3:
        unknown[0, 0] = known[0, 5 % m]
    if m >= 9 and n >= 3:  # query (0, n // 2) is exactly 1 away from known points 0, 1, 2, far from the cloud
        known[0, 0], known[0, 1], known[0, 2] = (21, 20, 20), (19, 20, 20), (20, 21, 20)
        unknown[0, n // 2] = (20, 20, 20)
    return unknown, known


# ------------------------------------------------------------------ restatements: numpy fp32 / float64
def decode_jitter_np32(inp):
    """calculate_bbox + the jitter in numpy float32: every operation individually rounded, like the
    tensor formulation (votenet_iou_branch.py:111-137, :157-172).  Also returns the branch decisions."""
    ns, nh = inp["size_scores"].shape[-1], inp["heading_scores"].shape[-1]
    mean = inp["mean_size"]
    sc = np.argmax(inp["size_scores"], -1)
    res = np.take_along_axis(inp["size_residuals"], sc[..., None, None], 2)[:, :, 0]
    raw = (mean[sc] + res) / F32(2)
    negative = raw < 0
    size = np.where(negative, TINY32, raw).astype(F32)
    hc = np.argmax(inp["heading_scores"], -1)
    hres = np.take_along_axis(inp["heading_residuals"], hc[..., None], 2)[..., 0]
    if nh == 1:
        heading, wrap = np.zeros(hc.shape, F32), np.zeros(hc.shape, bool)
    else:
        angle = hc.astype(F32) * F32(2 * np.pi / nh) + hres
        wrap = angle > PI32
        heading = (angle - wrap.astype(F32) * TWO_PI32).astype(F32)
    jc = inp["center"] + size * inp["noise_c"] * JITTER32
    js = size + size * inp["noise_s"] * JITTER32
    clamped = js < CLAMP32
    js = np.where(clamped, CLAMP32, js).astype(F32)
    out = {"size": size, "heading": heading, "jitter_center": jc.astype(F32), "jitter_size": js * F32(2),
           "jitter_heading": heading,
           "all_center": np.concatenate([inp["center"], jc], 1), "all_size": np.concatenate([size, js], 1),
           "all_heading": np.concatenate([heading, heading], 1)}
    assert all(v.dtype == F32 for v in out.values())
    return out, {"sc": sc, "hc": hc, "negative": negative, "wrap": wrap, "clamped": clamped}


def decode_jitter_f64(inp, size32, branch):
    """The same in float64 from the fp32 inputs, with the fp32 constants of the formulas and the branch
    decisions of the fp32 evaluation.  The jitter starts from the fp32 decoded size (`size32`, which is
    checked by itself), so its bound counts the jitter's own three roundings.  Returns values, bounds."""
    d = np.float64
    nh = inp["heading_scores"].shape[-1]
    mean = inp["mean_size"].astype(d)
    sc, hc = branch["sc"], branch["hc"]
    res = np.take_along_axis(inp["size_residuals"], sc[..., None, None], 2)[:, :, 0].astype(d)
    size = np.where(branch["negative"], d(TINY32), (mean[sc] + res) / 2)
    size_bound = 2 * EPS * (np.abs(mean[sc]) + np.abs(res))         # the sum and the halving
    hres = np.take_along_axis(inp["heading_residuals"], hc[..., None], 2)[..., 0].astype(d)
    if nh == 1:
        heading, heading_bound = np.zeros(hc.shape), np.zeros(hc.shape)
    else:
        base = hc.astype(d) * d(F32(2 * np.pi / nh))
        heading = base + hres - branch["wrap"] * d(TWO_PI32)
        heading_bound = 3 * EPS * (base + np.abs(hres) + d(TWO_PI32))  # product, sum, wrap
    s, c = size32.astype(d), inp["center"].astype(d)
    jc = c + s * inp["noise_c"].astype(d) * d(JITTER32)
    js = np.where(branch["clamped"], d(CLAMP32), s + s * inp["noise_s"].astype(d) * d(JITTER32))
    jc_bound = 4 * EPS * (np.abs(c) + np.abs(s) * (1 + np.abs(inp["noise_c"].astype(d))))
    js_bound = 4 * EPS * (np.abs(s) * (1 + np.abs(inp["noise_s"].astype(d))))
    return ({"size": size, "heading": heading, "jitter_center": jc, "jitter_size": 2 * js},
            {"size": size_bound, "heading": heading_bound, "jitter_center": jc_bound, "jitter_size": 2 * js_bound})


def unit_grid64():
    """the (64, 3) unit grid as torch computes it (fp32 linspace), x slowest / z fastest, as float64"""
    step = torch.linspace(-1, 1, 4).numpy().astype(np.float64)
    return np.stack(np.meshgrid(step, step, step, indexing="ij"), -1).reshape(64, 3)


def grid_f64(center, size, heading):
    """whole (b,k,64,3), relative (b,k,64,3) in float64 and their bounds (grid_conv_module.py:64-94)"""
    d = np.float64
    c, s, h = center.astype(d), size.astype(d), heading.astype(d)
    u = unit_grid64()
    local = u[None, None] * s[:, :, None, :]
    cos, sin = np.cos(h)[..., None], np.sin(h)[..., None]
    rel = np.stack([local[..., 0] * cos + local[..., 1] * sin, local[..., 1] * cos - local[..., 0] * sin,
                    local[..., 2]], -1)
    whole = rel + c[:, :, None, :]
    sx, sy, sz = (np.abs(s[..., i])[..., None] for i in range(3))
    ac = np.abs(c)[:, :, None, :]
    xy = 8 * EPS * (sx + sy)
    bw = np.stack([xy + 8 * EPS * ac[..., 0], xy + 8 * EPS * ac[..., 1], 2 * EPS * (sz + ac[..., 2])], -1)
    bw = np.broadcast_to(bw, whole.shape)
    # the relative rows: the same plus the rounding of the subtraction (|whole - c| <= sx + sy, sz)
    br = bw + EPS * np.broadcast_to(np.stack([sx + sy, sx + sy, sz], -1), whole.shape)
    return whole, rel, bw, br


def weights_np32(d2):
    """the kernel's documented arithmetic in numpy float32 (every operation IEEE-rounded): the weights with
    the sum taken as (w0 + w1) + w2, and the rows whose sum is the same in all three orders"""
    with np.errstate(divide="ignore"):
        r = F32(1) / (np.sqrt(d2) + CLAMP32)
    left = (r[..., 0] + r[..., 1]) + r[..., 2]
    right = r[..., 0] + (r[..., 1] + r[..., 2])
    outer = (r[..., 0] + r[..., 2]) + r[..., 1]
    order_free = (left == right) & (left == outer)
    return (r / left[..., None]).astype(F32), r, (left, right, outer), order_free


def weights_f64(d2):
    d = np.float64
    with np.errstate(divide="ignore"):
        w = 1.0 / (np.sqrt(d2.astype(d)) + d(CLAMP32))
    return w / w.sum(-1, keepdims=True)


# ------------------------------------------------------------------ helpers
def bits(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, dtype=F32).view(np.int32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r want %r" % (
            what, int(bad.sum()), bad.size, i, g.view(F32)[i], w.view(F32)[i]))


def assert_within(got, truth, bound, what):
    if torch.is_tensor(got):
        got = got.detach().cpu().numpy()
    err = np.abs(got.astype(np.float64) - truth)
    assert np.isfinite(got).all(), what
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s: max error %.3g, worst error / bound %.3f" % (what, float(err.max()) if err.size else 0.0, worst))
    assert (err <= bound).all(), (what, worst, int((err > bound).sum()))


def _mods(use_gpu, oracle, monkeypatch):
    load_pkg()
    utils = importlib.import_module("pointnet2.pointnet2_utils")
    V = importlib.import_module("3dioumatch_amd.votenet")
    if use_gpu:
        monkeypatch.setattr(utils, "_ext", importlib.import_module("pointnet2._ext"))
        return V, utils, torch.device("cuda:0")
    from oracle import standin
    monkeypatch.setattr(utils, "_ext", standin.make(oracle))
    return V, utils, torch.device("cpu")


def _tensor_path_only(monkeypatch):
    heads = importlib.import_module("3dioumatch_amd.votenet.heads")
    monkeypatch.setattr(heads, "_fused_front_end", lambda: None)


def run_jitter(V, tag, inp, dev, fused, monkeypatch):
    """VoteNet.forward_with_pred_jitter (and under it calculate_bbox / _bbox_jitter_fused), unbound, on a
    stub that carries what they read; the backbone returns the planted head outputs and the IoU branch is
    a recorder of the boxes it is given.  fused=False takes both switches of the tensor path."""
    cfgmod = importlib.import_module("3dioumatch_amd.votenet.config")
    ns, nh = CONFIGS[tag]
    b, k = inp["center"].shape[:2]
    cfg = cfgmod.DatasetConfig(NUM_CLASS[tag], nh, ns, mean_size_arr=inp["mean_size"])
    cfg.fused_heading_decode = bool(fused)
    if not fused:
        _tensor_path_only(monkeypatch)
    ep = {key: torch.from_numpy(inp[key]).to(dev) for key in
          ("center", "size_scores", "size_residuals", "heading_scores", "heading_residuals")}
    noise = (torch.from_numpy(inp["noise_c"]).to(dev), torch.from_numpy(inp["noise_s"]).to(dev))
    rec = {}

    def grid_conv(center, size, heading, end_points):
        rec.update(all_center=center, all_size=size, all_heading=heading)
        end_points["iou_scores"] = torch.zeros((b, center.shape[1], 1), device=dev)
        return end_points

    stub = types.SimpleNamespace(_mean_size=torch.from_numpy(inp["mean_size"]).to(dev), dataset_config=cfg,
                                 num_heading_bin=nh, grid_conv=grid_conv)
    stub.forward_backbone = lambda inputs: ep
    stub.calculate_bbox = lambda e: V.VoteNet.calculate_bbox(stub, e)
    stub._bbox_jitter_fused = lambda e, n=None: V.VoteNet._bbox_jitter_fused(stub, e, n)
    with torch.no_grad():
        out = V.VoteNet.forward_with_pred_jitter(stub, {"jitter_noise": noise})
    # the fused path hands out views of the kernel's (b, 2k, 3) tensor; the tensor path concatenates
    was_fused = out["jitter_center"].data_ptr() == rec["all_center"][:, k:].data_ptr()
    assert was_fused == (fused and dev.type == "cuda"), "the path under test was not taken"
    res = {key: out[key] for key in ("size", "heading", "jitter_center", "jitter_size", "jitter_heading")}
    res.update(rec)
    return res


class _Stop(Exception):
    pass


class _Recorder(nn.Module):
    """stands where GridConv.mlp_before_iou is: keeps the tensor the shared MLP would read and ends the
    forward there (the front end is what is under test)"""

    def forward_pooled(self, feats):
        self.feats = feats.detach().clone()
        raise _Stop()


def run_front_end(V, utils, center, size, heading, seeds, dev, fused, monkeypatch):
    """GridConv.forward up to the shared MLP: `whole` as three_nn receives it and the (b, 3+c, k, 64)
    tensor the shared MLP would read.  fused=False: heads.py's tensor formulation."""
    b, k = size.shape[:2]
    seed_xyz, seed_feats = seeds
    gc = V.GridConv(1, 1, 1, np.ones((1, 3), F32), k, "seed_fps", seed_feat_dim=seed_feats.shape[1])
    gc.mlp_before_iou = _Recorder()
    gc = gc.to(dev).eval()
    seen = {}
    real = utils._ext.three_nn

    def spy(unknown, known):
        seen["whole"] = unknown.detach().clone()
        return real(unknown, known)

    monkeypatch.setattr(utils._ext, "three_nn", spy)
    if not fused:
        _tensor_path_only(monkeypatch)
    as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    ep = {"seed_xyz": as_t(seed_xyz).to(dev), "seed_features": as_t(seed_feats).to(dev)}
    with torch.no_grad(), pytest.raises(_Stop):
        gc(as_t(center).to(dev), as_t(size).to(dev), as_t(heading).to(dev), ep)
    monkeypatch.setattr(utils._ext, "three_nn", real)
    feats = gc.mlp_before_iou.feats
    assert feats.shape == (b, 3 + seed_feats.shape[1], k, 64) and seen["whole"].shape == (b, k * 64, 3)
    return seen["whole"], feats[:, :3].reshape(b, 3, k * 64)


def call_grid_kernel(V, center, size, heading, ctot, dev):
    """votenet_gridconv_points as GridConv.forward calls it; feats is pre-filled with the sentinel"""
    L = importlib.import_module("3dioumatch_amd._lib")
    b, k = size.shape[:2]
    gc = V.GridConv(1, 1, 1, np.ones((1, 3), F32), k, "seed_fps", seed_feat_dim=16)
    c, s, h = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (center, size, heading))
    whole = torch.full((b, k * 64, 3), SENTINEL, dtype=torch.float32, device=dev)
    feats = torch.full((b, ctot, k * 64), SENTINEL, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib.votenet_gridconv_points(b, k, ctot, gc._unit_grid(dev).data_ptr(), c.data_ptr(),
                                              s.data_ptr(), h.data_ptr(), whole.data_ptr(), feats.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream),
                "votenet_gridconv_points")
    torch.cuda.synchronize()
    return whole, feats


def _xy_z(t):
    """(b, n, 3) points -> the x, y part and the z part"""
    return t[..., :2], t[..., 2]


# ------------------------------------------------------------------ builder sanity (CPU)
@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_builder_plants_the_edges(tag):
    """The planted proposals take the branches they are meant to take (decided in numpy float32)."""
    ns, nh = CONFIGS[tag]
    inp = head_inputs(tag, *GOLDEN_SHAPE)
    out, br = decode_jitter_np32(inp)
    p = inp["plants"]
    flat = lambda a: a.reshape((-1,) + a.shape[2:])  # noqa: E731
    t = p["size_neg_zero_negzero"]
    assert flat(br["sc"])[t] == ns - 1 and flat(br["sc"])[p["size_first_class"]] == 0
    assert list(bits(flat(out["size"])[t])) == list(bits(np.array([TINY32, 0.0, -0.0], F32)))
    assert flat(br["clamped"])[p["noise_at_clamp"]].all() and flat(br["clamped"])[p["noise_below_clamp"]].all()
    # away from the plants the clamp and the negative size stay rare
    assert br["clamped"].mean() < 0.1
    if nh > 1:
        h, w = flat(out["heading"]), flat(br["wrap"])
        assert h[p["heading_pi"]] == PI32 and not w[p["heading_pi"]]          # pi is NOT wrapped in fp32
        assert w[p["heading_pi_plus_ulp"]] and h[p["heading_pi_plus_ulp"]] < -3.14
        assert w[p["heading_last_wraps"]] and abs(h[p["heading_last_wraps"]]) < PI32
        assert w[p["heading_last_stays_above"]] and h[p["heading_last_stays_above"]] > PI32  # one subtraction
        assert not w[p["heading_first_negative"]] and h[p["heading_first_negative"]] == F32(-0.2)
        # in double the comparison at float32(pi) comes out the other way
        assert np.float64(F32(nh // 2) * F32(2 * np.pi / nh)) > np.pi
    ties = tie_rows(max(ns, 2))
    assert (ties == ties.max(-1, keepdims=True)).sum(-1).max() >= 2


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_tensor_path_is_the_fp32_formula_cpu(tag, shape, oracle, monkeypatch):
    """CPU: the package's tensor path (calculate_bbox + the jitter lines) == the numpy float32
    restatement, bit for bit, at every shape and configuration -- the restatement decides the branches of
    the float64 truth, so it is tied to the package's code here, without a GPU."""
    V, utils, dev = _mods(False, oracle, monkeypatch)
    inp = head_inputs(tag, *shape)
    got = run_jitter(V, tag, inp, dev, True, monkeypatch)
    want, _ = decode_jitter_np32(inp)
    for key, w in want.items():
        assert_bits(got[key], w, "%s %s" % (tag, key))


# ------------------------------------------------------------------ 2 + 3. bbox_jitter_kernel (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_bbox_jitter_kernel(tag, shape, ext, oracle, monkeypatch):
    """votenet_bbox_jitter == VoteNet.calculate_bbox + the jitter of forward_with_pred_jitter on the same
    device, bit for bit (only +, -, *, / of individually rounded operands), == the numpy float32
    restatement, and within the rounding-count bounds of the float64 truth."""
    V, utils, dev = _mods(True, oracle, monkeypatch)
    inp = head_inputs(tag, *shape)
    fused = run_jitter(V, tag, inp, dev, True, monkeypatch)
    tensor = run_jitter(V, tag, inp, dev, False, monkeypatch)
    np32, branch = decode_jitter_np32(inp)
    for key in np32:
        assert_bits(fused[key], tensor[key], "%s %s kernel vs tensor path" % (tag, key))
        assert_bits(fused[key], np32[key], "%s %s kernel vs numpy float32" % (tag, key))
    truth, bound = decode_jitter_f64(inp, np32["size"], branch)
    for key in truth:
        assert_within(fused[key], truth[key], bound[key], "%s %s vs float64" % (tag, key))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["scannet", "sunrgbd", "tiny"])
def test_bbox_jitter_argmax_takes_the_first_maximum(tag, ext, oracle, monkeypatch):
    """The kernel's contract on ties: arg-max = FIRST maximum (numpy.argmax's rule), for the size and the
    heading class.  The decoded size / heading name the class that was taken (every class decodes to a
    different value here).  What torch.argmax returns on the device for the same rows is recorded in the
    output (on the MI355X it took the first maximum in every row, like the kernel); exact ties between
    fp32 logits do not occur in a real pass and the tensor library does not specify its tie rule, so a
    difference there is reported, not asserted.  NaN scores are out of scope."""
    V, utils, dev = _mods(True, oracle, monkeypatch)
    ns, nh = CONFIGS[tag]
    srows, hrows = tie_rows(ns), tie_rows(nh)
    rows = max(len(srows), len(hrows))
    inp = head_inputs(tag, 1, rows, seed=3)
    inp["size_scores"][0] = srows[np.arange(rows) % len(srows)]
    inp["heading_scores"][0] = hrows[np.arange(rows) % len(hrows)]
    # class q decodes to sizes around q + 1 and to a heading residual of q / 100: all different
    inp["size_residuals"][0] = (2 * (np.arange(ns, dtype=F32) + 1))[None, :, None] - inp["mean_size"][None]
    inp["heading_residuals"][0] = (np.arange(nh, dtype=F32) / F32(100))[None]
    got = run_jitter(V, tag, inp, dev, True, monkeypatch)
    want, branch = decode_jitter_np32(inp)  # numpy.argmax: the first maximum
    assert len(np.unique(want["size"][0, :, 0])) == len(np.unique(branch["sc"]))
    assert_bits(got["size"], want["size"], "size class on ties")
    assert_bits(got["heading"], want["heading"], "heading class on ties")
    for name, scores, first in (("size", inp["size_scores"], branch["sc"]),
                                ("heading", inp["heading_scores"], branch["hc"])):
        on_device = torch.argmax(torch.from_numpy(scores).to(dev), -1).cpu().numpy()
        print("torch.argmax on the device, %s ties of %s: %d of %d rows differ from the first maximum%s" % (
            name, tag, int((on_device != first).sum()), first.size,
            "" if (on_device == first).all() else " (rows %s)" % np.argwhere(on_device != first)[:, 1].tolist()))


# ------------------------------------------------------------------ 2 + 3. gridconv_points_kernel (GPU)
@pytest.mark.gpu
def test_device_sincos_against_the_tensor_library(ext):
    """The one operation of the grid kernel that is not +, -, * or /: is the kernel's sinf / cosf the
    tensor library's sin / cos?  Isolated here: a box of half size (1, 0, 0) at the origin has its grid
    corner (x = 1) at (cos h, -sin h), each product with an exact 1 or 0.  Printed and asserted equal on
    the headings of part 1 -- if this ever fails, the x and y rows of the grid tests fail with it, and
    this test says why."""
    load_pkg()
    V = importlib.import_module("3dioumatch_amd.votenet")
    dev = torch.device("cuda:0")
    _, _, heading = grid_boxes(8, 512)
    center, size = np.zeros((8, 512, 3), F32), np.zeros((8, 512, 3), F32)
    size[..., 0] = 1.0
    whole, _ = call_grid_kernel(V, center, size, heading, 3, dev)
    corner = whole.view(8, 512, 64, 3)[:, :, 63]   # unit (1, 1, 1)
    h = torch.from_numpy(heading).to(dev)
    dc = bits(corner[..., 0]) != bits(torch.cos(h))
    ds = bits(corner[..., 1]) != bits(0 - torch.sin(h))
    print("device cosf vs torch.cos: %d of %d differ; sinf vs torch.sin: %d of %d differ" % (
        int(dc.sum()), dc.size, int(ds.sum()), ds.size))
    assert not dc.any() and not ds.any()


@pytest.mark.gpu
@pytest.mark.parametrize("ctot", [3, 3 + 256])
@pytest.mark.parametrize("shape", GRID_SHAPES, ids=lambda s: "%dx%d" % s)
def test_gridconv_points_kernel(shape, ctot, ext, oracle, monkeypatch):
    """votenet_gridconv_points == the tensor formulation of GridConv.forward (heads.py, the lines after
    the fused branch) on the same device, bit for bit: `whole` and the three relative rows; every other
    element of the wide tensor still holds the sentinel; and within the rounding-count bounds of the
    float64 truth."""
    V, utils, dev = _mods(True, oracle, monkeypatch)
    b, k = shape
    center, size, heading = grid_boxes(b, k)
    whole, feats = call_grid_kernel(V, center, size, heading, ctot, dev)
    want_whole, want_rel = run_front_end(V, utils, center, size, heading, seed_cloud(b, 64, 16), dev, False,
                                         monkeypatch)
    assert_bits(whole, want_whole, "whole")
    assert_bits(feats[:, :3], want_rel, "relative rows")
    if ctot > 3:
        rest = bits(feats[:, 3:])
        assert (rest == bits(np.array([SENTINEL], F32))[0]).all(), "the kernel wrote outside rows 0..2"
    w64, r64, bw, br = grid_f64(center, size, heading)
    assert_within(whole.view(b, k, 64, 3), w64, bw, "whole vs float64")
    assert_within(feats[:, :3].view(b, 3, k, 64).permute(0, 2, 3, 1), r64, br, "relative vs float64")


# ------------------------------------------------------------------ 2 + 3. three_nn_weights_kernel (GPU)
WEIGHT_CLOUDS = [(2, 1, 64), (2, 255, 64), (2, 256, 64), (2, 257, 64), (2, 9216, 64), (2, 257, 2),
                 (2, 257, 1), (1, 1, 1), (8, 32768, 1024)]


@pytest.mark.gpu
def test_library_sum_of_three_is_not_a_fixed_order(ext):
    """The one operation of the weight formula that the tensor library does not fix: torch.sum over the
    three neighbours.  Isolated here on IEEE-exact inputs (sqrt, + 1e-8, reciprocal and the final division
    of the library are each bit-equal to IEEE fp32 on this stack, asserted below; the sum is not the
    kernel's: on the MI355X it equals (w0 + w1) + w2 in 13499, w0 + (w1 + w2) in 14211 and (w0 + w2) + w1 in
    all 18432 of 18432 rows; torch on the CPU adds in yet another order).  Asserted: where all orders round
    alike the library agrees, and it is within two roundings of the exact sum.  Printed: how many rows it
    shares with each order.  Which order the library takes is its own business and is not asserted."""
    dev = torch.device("cuda:0")
    unknown, known = nn_clouds(2, 9216, 64)
    d2, _ = ext.three_nn(torch.from_numpy(unknown).to(dev), torch.from_numpy(known).to(dev))
    d2n = d2.cpu().numpy()
    _, r, orders, order_free = weights_np32(d2n)
    finite = np.isfinite(r).all(-1)
    lib = torch.sum(torch.from_numpy(r).to(dev), dim=2).cpu().numpy()
    for name, o in zip(("(w0+w1)+w2", "w0+(w1+w2)", "(w0+w2)+w1"), orders):
        print("torch.sum(dim=2) on the device == %s in %d of %d rows" % (
            name, int((bits(lib) == bits(o)).sum()), lib.size))
    assert (bits(lib)[order_free] == bits(orders[0])[order_free]).all()
    exact = r.astype(np.float64).sum(-1)
    assert (np.abs(lib[finite] - exact[finite]) <= 2 * EPS * exact[finite]).all()
    for op, mine, ieee in (("sqrt", torch.sqrt(d2), np.sqrt(d2n)),
                           ("reciprocal", 1.0 / (torch.sqrt(d2) + 1e-8), r)):
        assert_bits(mine, ieee, "the library's %s against IEEE fp32" % op)


@pytest.mark.gpu
@pytest.mark.parametrize("cloud", WEIGHT_CLOUDS, ids=lambda c: "%dx%dx%d" % c)
def test_three_nn_weights_kernel(cloud, ext, oracle, monkeypatch):
    """pn2_three_nn_weights on the distances of the real three_nn == 1 / (sqrt(d2) + 1e-8) / sum as
    three_nn_with_weights writes it with tensor operations, bit for bit, rows with +inf (fewer than three
    known points) and with zeros (a query on a known point) included, no NaN; within 8 * 2^-24 of the
    float64 value, rows summing to 1 within 4 * 2^-24; and within 16 * 2^-24 of the reference's formula,
    which recomputes the distances from the gathered seeds (grid_conv_module.py:89-99)."""
    V, utils, dev = _mods(True, oracle, monkeypatch)
    b, n, m = cloud
    unknown, known = nn_clouds(b, n, m)
    u, kn = torch.from_numpy(unknown).to(dev), torch.from_numpy(known).to(dev)
    d2, idx = ext.three_nn(u, kn)
    got_idx, got = utils.three_nn_with_weights(u, kn)
    assert got.shape == (b, n, 3) and torch.equal(got_idx, idx)
    assert_bits(got, ext.three_nn_weights(d2), "wrapper vs entry point")
    with monkeypatch.context() as mp:  # three_nn followed by the tensor operations
        mp.setattr(ext, "three_nn_weights", None)
        want_idx, want = utils.three_nn_with_weights(u, kn)
    assert torch.equal(want_idx, idx)
    d2n, gotn = d2.cpu().numpy(), got.cpu().numpy()
    assert not np.isnan(gotn).any() and not torch.isnan(want).any()
    assert np.isinf(d2n).any() == (m < 3) and (d2n[0, 0, 0] == 0)
    if m >= 3:
        assert (d2n[b - 1, n - 1, :2] == 0).all() and d2n[b - 1, n - 1, 2] > 0
    # the kernel's own contract: each operation rounded to fp32, the sum as (w0 + w1) + w2 -- every row
    np32, _, _, order_free = weights_np32(d2n)
    assert_bits(got, np32, "weights vs the IEEE fp32 evaluation of the documented order")
    # the tensor formulation: torch.sum over the three neighbours adds in an order of its own on this
    # stack (test_library_sum_of_three_is_not_a_fixed_order), so the normalised weights are bit-equal
    # where the order cannot matter -- one finite neighbour, three equal distances, any row whose three
    # orders round alike -- and within the float64 bound of part 3 elsewhere
    assert order_free[np.isinf(d2n[..., 1])].all()
    if m >= 9 and n >= 3:
        assert (d2n[0, n // 2] == 1).all() and order_free[0, n // 2]
    assert n < 255 or order_free.mean() > 0.2  # (the part of the rows held to bit equality)
    assert_bits(got[torch.from_numpy(order_free).to(dev)], want[torch.from_numpy(order_free).to(dev)],
                "weights vs tensor formulation, rows whose sum has one value in any order")
    assert_within(gotn, want.cpu().numpy().astype(np.float64), np.full(gotn.shape, 8 * EPS),
                  "weights vs tensor formulation, all rows")
    truth = weights_f64(d2n)
    assert_within(gotn, truth, np.full(truth.shape, 8 * EPS), "weights vs float64")
    assert np.abs(gotn.astype(np.float64).sum(-1) - 1).max() <= 4 * EPS
    # a query ON one known point: that neighbour takes (nearly) all the weight
    one_zero = (d2n[..., 0] == 0) & (d2n[..., 1] > 0.05 ** 2)
    assert one_zero.any() or (b, n) == (1, 1)
    assert (np.abs(gotn[one_zero][:, 0].astype(np.float64) - 1) <= 2.0 ** -20).all()
    if m >= 3:  # (with fewer known points the reference's gather would re-read seed 0 for the missing ones)
        kn64, u64 = known.astype(np.float64), unknown.astype(np.float64)
        picked = np.stack([kn64[i][idx[i].cpu().numpy().astype(np.int64)] for i in range(b)])  # (b,n,3,3)
        dist = np.sqrt(((picked - u64[:, :, None]) ** 2).sum(-1))
        ref = 1.0 / (dist + 1e-8)
        ref = ref / ref.sum(-1, keepdims=True)
        assert_within(gotn, ref, np.full(ref.shape, 16 * EPS), "weights vs the reference's formula")


# ------------------------------------------------------------------ 4. the reference at the same edges
def _golden_inputs(g, tag):
    inp = {key: g["%s_in::%s" % (tag, key)] for key in
           ("center", "size_scores", "size_residuals", "heading_scores", "heading_residuals", "noise_c",
            "noise_s", "mean_size")}
    built = head_inputs(tag, *GOLDEN_SHAPE)
    for key in inp:  # the fixture was made from THIS builder; only the noise was drawn by torch
        if key not in ("noise_c", "noise_s"):
            assert_bits(inp[key], built[key], "builder drifted from the fixture: " + key)
    planted_c, planted_s = inp["noise_c"].copy(), inp["noise_s"].copy()
    plant_noise(planted_c, planted_s, built["plants"])
    assert_bits(planted_c, inp["noise_c"], "planted centre noise")
    assert_bits(planted_s, inp["noise_s"], "planted size noise")
    return inp


@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
@pytest.mark.parametrize("use_gpu", [pytest.param(False, id="cpu-tensor-path"),
                                     pytest.param(True, id="gpu-kernels", marks=pytest.mark.gpu)])
def test_front_end_matches_reference(use_gpu, tag, oracle, monkeypatch):
    """The REFERENCE's VoteNet.forward_with_pred_jitter and GridConv.forward on the planted head outputs
    (iou_front_ref.npz): decoded and jittered boxes bit for bit; the grid points the reference hands to
    three_nn and the relative rows it hands to its shared MLP within the rounding-count bound (the
    reference rotates with torch.bmm, whose summation order is the BLAS library's).  CPU: this package's
    tensor path.  GPU: the fused kernels."""
    V, utils, dev = _mods(use_gpu, oracle, monkeypatch)
    g = golden("iou_front_ref.npz")
    inp = _golden_inputs(g, tag)
    b, k = GOLDEN_SHAPE
    got = run_jitter(V, tag, inp, dev, True, monkeypatch)
    for key in ("size", "heading", "jitter_center", "jitter_size", "jitter_heading"):
        assert_bits(got[key], g["%s_%s" % (tag, key)], "%s %s vs the reference" % (tag, key))
    seeds = (g[tag + "_in::seed_xyz"], g[tag + "_in::seed_features"])
    whole, rel = run_front_end(V, utils, got["all_center"], got["all_size"], got["all_heading"], seeds, dev,
                               True, monkeypatch)
    boxes = g[tag + "_grid_boxes"].astype(np.int64)  # flat indices into the (b, 2k) boxes
    bi, ki = boxes // (2 * k), boxes % (2 * k)
    c, s, h = (got[key].cpu().numpy() for key in ("all_center", "all_size", "all_heading"))
    _, _, bw, br = grid_f64(c, s, h)
    whole = whole.view(b, 2 * k, 64, 3).cpu().numpy()[bi, ki]
    rel = rel.view(b, 3, 2 * k, 64).permute(0, 2, 3, 1).cpu().numpy()[bi, ki]
    assert_within(whole, g[tag + "_whole"].astype(np.float64), bw[bi, ki], tag + " whole vs the reference")
    assert_within(rel, g[tag + "_relative"].astype(np.float64), br[bi, ki], tag + " relative vs the reference")
    # z: lz + cz and its difference are single exact-rounded operations on either side
    assert_bits(whole[..., 2], g[tag + "_whole"][..., 2], tag + " whole z vs the reference")
    assert_bits(rel[..., 2], g[tag + "_relative"][..., 2], tag + " relative z vs the reference")


# ------------------------------------------------------------------ 5. the paths of the module agree
def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _close_to_range(got, want, tol, what):
    got, want = got.detach().float().cpu().numpy(), want.detach().float().cpu().numpy()
    err, scale = float(np.abs(got - want).max()), max(1.0, float(np.abs(want).max()))
    print("%s: max error %.3g of range %.3g" % (what, err, scale))
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["scannet", "sunrgbd"])
def test_detector_paths_agree(tag, ext, oracle, monkeypatch):
    """VoteNet.forward_with_pred_jitter at the train-step golden's B, K, N with seeded weights and a given
    jitter noise: as shipped (votenet_bbox_jitter + the fused GridConv front end) against the tensor path
    of the same module (dataset_config.fused_heading_decode = False, heads._fused_front_end -> None) on
    the SAME head outputs.  Decoded and jittered boxes bit for bit; in eval mode the IoU scores within 2e-4
    of their range (test_gpu_mlp.py's tolerance for a fused chain's forward output)."""
    from make_layer_golden import seeded_state
    from make_step_golden import B, K, N
    V, utils, dev = _mods(True, oracle, monkeypatch)
    data = importlib.import_module("3dioumatch_amd.votenet.data")
    cfg = V.scannet_config() if tag == "scannet" else V.sunrgbd_config()
    net = V.VoteNet(cfg.num_class, cfg.num_heading_bin, cfg.num_size_cluster, cfg.mean_size_arr, cfg,
                    input_feature_dim=1, num_proposal=K, sampling="seed_fps")
    net = seeded_state(net, seed=21).to(dev).eval()
    batch = data.make_batch(B, N, cfg, seed=33, num_objects=6)
    g = torch.Generator().manual_seed(5)
    noise_c, noise_s = torch.randn(B, K, 3, generator=g).numpy(), torch.randn(B, K, 3, generator=g).numpy()
    plant_noise(noise_c, noise_s, plant_positions(cfg.num_heading_bin, B * K))
    inputs = {"point_clouds": batch["point_clouds"].to(dev),
              "jitter_noise": (torch.from_numpy(noise_c).to(dev), torch.from_numpy(noise_s).to(dev))}
    kept = {}
    backbone = net.forward_backbone

    def recording_backbone(inp):
        kept.update(backbone(inp))
        return dict(kept)

    monkeypatch.setattr(net, "forward_backbone", recording_backbone)
    with torch.no_grad():
        shipped = net.forward_with_pred_jitter(inputs)
        assert shipped["jitter_center"]._base is not None  # a view of the kernel's (B, 2K, 3) tensor
        monkeypatch.setattr(net, "forward_backbone", lambda inp: dict(kept))
        monkeypatch.setattr(cfg, "fused_heading_decode", False, raising=False)
        _tensor_path_only(monkeypatch)
        tensor = net.forward_with_pred_jitter(inputs)
        assert tensor["jitter_center"]._base is None
    for key in ("size", "heading", "jitter_center", "jitter_size", "jitter_heading"):
        assert_bits(shipped[key], tensor[key], "%s %s fused vs tensor path" % (tag, key))
    if tag == "sunrgbd":
        assert float(shipped["heading"].abs().max()) > 0
    for key in ("iou_scores", "iou_scores_jitter"):
        assert shipped[key].shape == tensor[key].shape == (B, K, cfg.num_class)
        _close_to_range(shipped[key], tensor[key], 2e-4, "%s %s fused vs tensor path" % (tag, key))


def _grid_conv(V, k, dev, training):
    from make_layer_golden import seeded_state
    mean = mean_size_table(18)
    gc = V.GridConv(18, 1, 18, mean, k, "seed_fps")
    return seeded_state(gc, seed=11).to(dev).train(training)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 40), (8, 512)], ids=lambda s: "%dx%d" % s)
def test_gridconv_three_paths(shape, ext, oracle, monkeypatch):
    """GridConv.forward in eval mode, 1024 seeds x 256 channels: (a) the fused front end with the first
    layer commuted with the interpolation, (b) PN2_INTERP_FIRST=0, (c) the recording path that
    evaluate_with_opt differentiates (center and size with requires_grad).  Grid points and neighbour
    indices are identical in all three.  Truth: path (c)'s tensor operations in float64 on the CPU with the
    device's indices.  test_gpu_mlp.py's _grad_bound rule: the error of (a) and of (b) is at most
    2e-4 + 3 x the error of (c), relative norms.  Train mode, (a) against (b): the running statistics of
    the five BatchNorm layers within rtol 1e-4 / atol 1e-5."""
    import copy
    V, utils, dev = _mods(True, oracle, monkeypatch)
    b, k = shape
    center, size, heading = (torch.from_numpy(a).to(dev) for a in grid_boxes(b, k, seed=1, sane=True))
    xyz, feats = (torch.from_numpy(a).to(dev) for a in seed_cloud(b, 1024, 256, seed=1))
    gc = _grid_conv(V, k, dev, False)
    seen = []
    real = utils._ext.three_nn

    def spy(unknown, known):
        out = real(unknown, known)
        seen.append((unknown.detach().clone(), out[1].clone()))
        return out

    monkeypatch.setattr(utils._ext, "three_nn", spy)
    commuted = []
    interp = gc.mlp_before_iou.forward_pooled_interp
    monkeypatch.setattr(gc.mlp_before_iou, "forward_pooled_interp",
                        lambda *a, **kw: commuted.append(1) or interp(*a, **kw))

    def run(module, mode):
        ep = {"seed_xyz": xyz, "seed_features": feats}
        if mode == "c":
            c, s = center.clone().requires_grad_(True), size.clone().requires_grad_(True)
            return module(c, s, heading, ep)["iou_scores"].detach()
        with torch.no_grad():
            return module(center, size, heading, ep)["iou_scores"]

    out_a = run(gc, "a")
    assert commuted == [1]
    with monkeypatch.context() as mp:
        mp.setenv("PN2_INTERP_FIRST", "0")
        out_b = run(gc, "b")
    assert commuted == [1]
    out_c = run(gc, "c")
    assert len(seen) == 3
    for other in seen[1:]:
        assert_bits(other[0], seen[0][0], "grid points of the three paths")
        assert torch.equal(other[1], seen[0][1])
    monkeypatch.setattr(utils._ext, "three_nn", real)

    # float64 truth, one cloud at a time (eval mode: the clouds are independent)
    twin = copy.deepcopy(gc).double().cpu().eval()
    idx = seen[0][1].cpu()
    truth = []
    for i in range(b):
        stub = types.SimpleNamespace(three_nn=lambda u, kn, i=i: [torch.zeros(1, u.shape[1], 3, dtype=u.dtype),
                                                                  idx[i:i + 1]])
        with monkeypatch.context() as mp:
            mp.setattr(utils, "_ext", stub)
            ep = {"seed_xyz": xyz[i:i + 1].double().cpu(), "seed_features": feats[i:i + 1].double().cpu()}
            c = center[i:i + 1].double().cpu().requires_grad_(True)
            truth.append(twin(c, size[i:i + 1].double().cpu(), heading[i:i + 1].double().cpu(),
                              ep)["iou_scores"].detach())
    truth = torch.cat(truth)
    assert truth.dtype == torch.float64 and truth.shape == out_a.shape == (b, k, 18)
    e_a, e_b, e_c = _rel(out_a, truth), _rel(out_b, truth), _rel(out_c, truth)
    print("GridConv %dx%d vs float64: commuted %.3g, materialised %.3g, recording path %.3g" % (b, k, e_a, e_b, e_c))
    assert e_a <= 2e-4 + 3 * e_c and e_b <= 2e-4 + 3 * e_c, (e_a, e_b, e_c)

    stats = []
    for interp_first in ("1", "0"):
        module = _grid_conv(V, k, dev, True)
        with monkeypatch.context() as mp:
            mp.setenv("PN2_INTERP_FIRST", interp_first)
            run(module, "a")
        stats.append({n: t.clone() for n, t in module.named_buffers()})
    names = [n for n in stats[0] if n.endswith("running_mean") or n.endswith("running_var")]
    assert len(names) == 10
    for n in names:
        assert torch.allclose(stats[0][n], stats[1][n], rtol=1e-4, atol=1e-5), n
        assert not torch.equal(stats[0][n], _grid_conv(V, k, "cpu", True).state_dict()[n].to(dev)), n  # it moved


@pytest.mark.gpu
def test_fp_module_with_fused_weights(ext, oracle, monkeypatch):
    """PointnetFPModule at the backbone's shapes (1024 -> 2048 points, 256 + 256 channels), eval mode:
    three_nn_with_weights through the weight kernel against three_nn followed by the tensor operations
    (_ext.three_nn_weights patched away).  Indices identical; weights as in
    test_three_nn_weights_kernel; the module's output bit-equal in every column whose weights are
    (a 1x1 shared MLP treats the points independently), and within 2e-4 of its range everywhere."""
    from make_layer_golden import seeded_state
    V, utils, dev = _mods(True, oracle, monkeypatch)
    mods = importlib.import_module("pointnet2.pointnet2_modules")
    b, n, m = 2, 2048, 1024
    unknown, known = nn_clouds(b, n, m, seed=2)
    g = np.random.default_rng(2)
    u, kn = torch.from_numpy(unknown).to(dev), torch.from_numpy(known).to(dev)
    uf = torch.from_numpy(g.standard_normal((b, 256, n)).astype(F32)).to(dev)
    kf = torch.from_numpy(g.standard_normal((b, 256, m)).astype(F32)).to(dev)
    fp = seeded_state(mods.PointnetFPModule(mlp=[256 + 256, 256, 256]), seed=4).to(dev).eval()
    with torch.no_grad():
        idx_f, w_f = utils.three_nn_with_weights(u, kn)
        out_f = fp(u, kn, uf, kf)
        with monkeypatch.context() as mp:
            mp.setattr(ext, "three_nn_weights", None)
            idx_t, w_t = utils.three_nn_with_weights(u, kn)
            out_t = fp(u, kn, uf, kf)
    assert torch.equal(idx_f, idx_t)
    d2, _ = ext.three_nn(u, kn)
    _, _, _, order_free = weights_np32(d2.cpu().numpy())
    same = torch.from_numpy((bits(w_f) == bits(w_t)).all(-1)).to(dev)          # (b, n) points
    assert bool(same[torch.from_numpy(order_free).to(dev)].all()) and float(same.float().mean()) > 0.2
    assert_within(w_f, w_t.cpu().numpy().astype(np.float64), np.full(tuple(w_f.shape), 8 * EPS),
                  "FP weights, kernel vs tensor operations")
    assert out_f.shape == (b, 256, n)
    cols = same.unsqueeze(1).expand_as(out_f)
    assert_bits(out_f[cols], out_t[cols], "FP output at the points whose weights are bit-equal")
    _close_to_range(out_f, out_t, 2e-4, "FP output")


# ------------------------------------------------------------------ 6. argument checks (no launch)
INVALID = 1  # hipErrorInvalidValue


@pytest.mark.gpu
def test_entry_points_reject_bad_arguments(ext):
    """Invalid arguments are rejected on the host with hipErrorInvalidValue before any launch; an empty
    batch returns 0.  Every pointer handed over is either null or a live device buffer large enough for
    the shape that is passed, and the oversized grid has b*k*64 == 2^32 (no lane would be in range)."""
    L = importlib.import_module("3dioumatch_amd._lib")
    dev = torch.device("cuda:0")
    buf = [torch.zeros(4096, device=dev) for _ in range(15)]
    p = [t.data_ptr() for t in buf]
    grid = L.lib.votenet_gridconv_points
    assert grid(1, 1, 2, p[0], p[1], p[2], p[3], p[4], p[5], None) == INVALID          # ctot = 2
    for hole in range(6):
        args = list(p[:6]); args[hole] = None
        assert grid(1, 1, 3, *args, None) == INVALID, hole                               # a null pointer
    assert grid(32768, 2048, 3, *p[:6], None) == INVALID                                 # b*k*64 > 2^31 - 1
    assert grid(0, 4, 3, *p[:6], None) == 0 and grid(0, 4, 3, *([None] * 6), None) == 0
    jit = L.lib.votenet_bbox_jitter
    assert jit(1, 1, 0, 1, *p[:14], None) == INVALID                                     # ns = 0
    args = list(p[:14]); args[3] = args[4] = None
    assert jit(1, 1, 2, 12, *args, None) == INVALID                                      # nh = 12, no heading
    assert jit(1, 1, 2, 0, *p[:14], None) == INVALID                                     # nh = 0
    assert jit(0, 4, 2, 12, *p[:14], None) == 0
    wts = L.lib.pn2_three_nn_weights
    assert wts(4, None, p[0], None) == INVALID and wts(4, p[0], None, None) == INVALID
    assert wts(0, p[0], p[1], None) == 0
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0 for t in buf), "something was launched"
