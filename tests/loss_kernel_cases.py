"""Inputs and float64 truth for tests/test_loss_kernels.py (no network, no package import).

  build(shape, ...)   seeded labels, head outputs, mean sizes and planted IoU labels of one shape
                      (B, K, G, S, VF, N, NH, NS, NC, NI, jitter, layout) with the edges listed in
                      `build`'s docstring; every float is an fp32 value, so the kernels and the float64
                      evaluation read identical numbers.  The builder asserts in float64 that no label
                      hangs on a rounding (margins()), and moves offending points by a fixed rule first.
  reference(case)     models/loss_helper_labeled.py:28-370 (and the consistency mode of
                      loss_helper_unlabeled.py:292-361) in torch float64, written from the formulas and not
                      from votenet/losses.py (which casts to float32): labels, statistics, decoded boxes
                      with their rounding-count bounds, and by autograd the gradient of the loss with
                      respect to every head output and the votes.
"""
import functools

import numpy as np
import torch

F32 = np.float32
EPS = 2.0 ** -24  # the relative error of ONE fp32 rounding
NEAR, FAR = 0.3, 0.6
SHIFT = np.array([0.013, -0.007, 0.005], F32)  # the fixed move of an offending point

# (B, K, G, S, VF, N, NH, NS, NC, NI, jitter, layout): each the smallest shape at which its path exists
CASES = {
    # a full proposal block, four seed blocks (the benchmark's K and S)
    "workload_block": (2, 256, 64, 1024, 1, 1500, 1, 18, 18, 18, True, "strided"),
    # two proposal blocks with a partial one; 5 * (2 + 1 + 2) = 25 partial rows, not a multiple of 8
    "second_block": (5, 300, 70, 300, 1, 500, 12, 10, 10, 10, True, "contiguous"),
    # one live lane in the last proposal and seed blocks; two votes per seed
    "one_lane_over": (3, 257, 64, 257, 2, 400, 1, 18, 18, 18, True, "strided"),
    # three blocks; G = kMaxG (the GT workgroup's stride loop runs its full length, gtc filled); rows wider
    # than kRowMax = 32 in all three class heads; one IoU channel
    "limits_wide_rows": (2, 513, 256, 40, 1, 64, 33, 40, 37, 1, False, "strided"),
    # ctr[kMaxK * 3] filled; eight proposal blocks; one ground-truth slot
    "k_limit": (1, 2048, 1, 1, 1, 4, 2, 1, 1, 1, False, "contiguous"),
    "smallest": (1, 1, 1, 1, 1, 1, 2, 1, 1, 1, False, "contiguous"),
}
CONSISTENCY_CASES = ("workload_block", "second_block", "one_lane_over", "limits_wide_rows")
SCALED = ("second_block",)  # grad_scale = 0.37 there, in both modes

HEADS3 = ("obj", "center", "h_scores", "h_resn", "s_scores", "sem", "iou", "iou_jit")
GRAD_OF = {"g_obj": "obj", "g_center": "center", "g_h_scores": "h_scores", "g_h_resn": "h_resn",
           "g_s_scores": "s_scores", "g_s_resn": "s_resn", "g_sem": "sem", "g_iou": "iou",
           "g_iou_jit": "iou_jit", "g_vote": "vote_xyz"}


# ------------------------------------------------------------------ margins (float64)
def _two_smallest(d):
    """(..., n) -> smallest, second smallest, arg of the second; n == 1: second = +inf"""
    if d.shape[-1] == 1:
        return d[..., 0], np.full(d.shape[:-1], np.inf), np.zeros(d.shape[:-1], np.int64)
    order = np.argsort(d, axis=-1, kind="stable")[..., :2]
    two = np.take_along_axis(d, order, -1)
    return two[..., 0], two[..., 1], order[..., 1]


def _tied(first, second):
    return (second - first) < 1e-5 * np.maximum(second, 1e-300)


def _candidates(c, b):
    """GT slots of scene b as arg-min candidates: the valid ones and ONE of the empty ones (they are
    identical points, asserted in build(): an exact tie between them resolves to the first index)"""
    valid = c["box_label_mask"][b] == 1
    cols = list(np.flatnonzero(valid))
    if (~valid).any():
        cols.append(int(np.flatnonzero(~valid)[0]))
    return np.array(cols)


def margins(c):
    """Every label decision of the loss with less than the required margin: a list of (kind, b, index,
    other).  Required: sqrt(d2 + 1e-6) at least 1e-4 from 0.3 and 0.6; the smallest and second-smallest
    candidate of every arg-min at least 1e-5 apart, relative."""
    d = np.float64
    bad = []
    B = c["center_label"].shape[0]
    raw = c["center_label"].astype(d)
    masked = np.where((c["box_label_mask"] == 1)[..., None], raw, -1000.0)
    for b in range(B):
        cols = _candidates(c, b)
        # vote -> valid GT centre
        d2 = ((c["agg_xyz"][b].astype(d)[:, None] - masked[b][None, cols]) ** 2).sum(-1)
        first, second, _ = _two_smallest(d2)
        dist = np.sqrt(first + 1e-6)
        off = _tied(first, second) | (np.abs(dist - NEAR) < 1e-4) | (np.abs(dist - FAR) < 1e-4)
        bad += [("agg", b, int(k), -1) for k in np.flatnonzero(off)]
        # centre -> GT centre (raw labels, padded slots included)
        dc = ((c["center"][b].astype(d)[:, None] - raw[b][None, cols]) ** 2).sum(-1)
        first, second, _ = _two_smallest(dc)
        bad += [("center", b, int(k), -1) for k in np.flatnonzero(_tied(first, second))]
        # GT centre -> centre
        dg = ((raw[b][:, None] - c["center"][b].astype(d)[None]) ** 2).sum(-1)
        first, second, arg2 = _two_smallest(dg)
        bad += [("gt", b, int(g), int(arg2[g])) for g in np.flatnonzero(_tied(first, second))]
    if c["S"]:
        first, second, _ = _two_smallest(_vote_distances(c))
        bad += [("vote", int(b), int(s), -1) for b, s in np.argwhere(_tied(first, second))]
    return bad


def _vote_distances(c):
    """(B, S, VF * 3) L1 distances of every (vote, GT vote) pair of a seed, float64"""
    d = np.float64
    B, S, VF = c["B"], c["S"], c["VF"]
    inds = c["seed_inds"].astype(np.int64)
    gt = np.take_along_axis(c["vote_label"].astype(d), inds[..., None], 1).reshape(B, S, 1, 3, 3)
    gt = gt + c["seed_xyz"].astype(d).reshape(B, S, 1, 1, 3)
    votes = c["vote_xyz"].astype(d).reshape(B, S, VF, 1, 3)
    return np.abs(votes - gt).sum(-1).reshape(B, S, VF * 3)


def _separate_top(rows):
    """arg-max of a score row must not hang on a rounding: where the two largest scores are closer than
    1e-4 the largest is raised by 0.01"""
    if rows.shape[-1] < 2:
        return
    flat = rows.reshape(-1, rows.shape[-1])
    order = np.argsort(flat, -1)
    top, second = order[:, -1], order[:, -2]
    r = np.arange(flat.shape[0])
    close = (flat[r, top].astype(np.float64) - flat[r, second]) < 1e-4
    flat[r[close], top[close]] += F32(0.01)


# ------------------------------------------------------------------ the builder
@functools.lru_cache(maxsize=None)
def build(name, consistency=False, no_positive=False, seed=0):
    """The inputs of case `name` as a dict of numpy arrays (treat as read-only: shared between tests).

    Placement (every scene but the empty one): a third of the aggregated votes ~0.1 m from a valid GT
    centre, a third ~0.45 m (the ignored band), the rest ~0.9 m; GT centres 2.5 m apart on a grid.
    Planted:
      * B > 1: the FIRST scene has every slot empty (assignment 0 = the first minimum, no positive); the
        other planted proposals sit in the LAST scene, so that the last partial rows (its GT workgroup's, and
        the last seed workgroup's: seed S-1 is an object seed) carry sums that a dropped row would miss;
      * slot G-1 (and, G >= 2, slot G//2, 1.5 m from it) sit 20 m from everything else with ONE proposal,
        K-1, next to them: both slots share that nearest proposal, it is a positive, and for K > 256 its
        index is >= 256 (another workgroup than the one that stages the slot);
      * last scene, on positives: objectness scores (40, -40) and (-40, 40), class scores of +-60 in the
        semantic / size / heading heads, heading and size residuals off by more than 1 in both signs, a
        size residual of -1.5 (decoded size <= 0 -> 1e-6), the last heading class with a residual that wraps
        past pi; on a negative: objectness (-40, 40);
      * IoU labels of exactly 0 and 1.
    consistency: the pseudo-label layout (empty slots' centres at -1000, S = VF = 0, one IoU channel unused).
    no_positive: every aggregated vote 50 m away and every vote_label_mask zero."""
    B, K, G, S, VF, N, NH, NS, NC, NI, jitter, layout = CASES[name]
    if consistency:
        S = VF = N = 0
        jitter = False
    rng = np.random.default_rng([seed, B, K, G, S, VF, N, NH, NS, NC, NI, int(jitter)])
    f = lambda a: np.ascontiguousarray(a, dtype=F32)  # noqa: E731
    c = dict(name=name, B=B, K=K, G=G, S=S, VF=VF, N=N, NH=NH, NS=NS, NC=NC, NI=NI, jitter=jitter,
             layout=layout, consistency=consistency, no_positive=no_positive)

    # ---- ground truth
    side = int(np.ceil(G ** (1 / 3)))
    cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    center_label = np.zeros((B, G, 3))
    mask = np.zeros((B, G), F32)
    g1, g2 = G - 1, (G // 2 if G >= 2 else None)
    empty_scene, ps = (0 if B > 1 else None), B - 1  # ps: the scene of the planted proposals
    for b in range(B):
        if b == empty_scene:
            continue
        center_label[b] = 3.0 + 2.5 * cells[rng.permutation(len(cells))[:G]] + rng.uniform(-0.2, 0.2, (G, 3))
        valid = rng.random(G) < 0.6
        if G >= 4:
            valid[0], valid[1] = (b != ps), True  # the planted scene: the first slot is an empty one
        valid[g1] = True
        center_label[b, g1] = -20.0 - b
        if g2 is not None:
            valid[g2] = True
            center_label[b, g2] = center_label[b, g1] + (1.5, 0, 0)
        mask[b] = valid
        center_label[b, ~valid] = 0.0  # what the loaders pad with
    if consistency:
        center_label[mask != 1] = -1000.0
    c["center_label"], c["box_label_mask"] = f(center_label), mask
    c["mean_size"] = f(rng.uniform(0.4, 1.8, (NS, 3)))
    c["heading_class_label"] = rng.integers(0, NH, (B, G)).astype(np.int64)
    c["heading_residual_label"] = f(rng.uniform(-0.9, 0.9, (B, G)) * np.pi / NH)
    c["size_class_label"] = rng.integers(0, NS, (B, G)).astype(np.int64)
    c["size_residual_label"] = f(rng.uniform(-0.2, 0.2, (B, G, 3)))
    c["sem_cls_label"] = rng.integers(0, NC, (B, G)).astype(np.int64)

    # ---- proposals
    agg = rng.uniform(2, 12, (B, K, 3))
    cls = np.full((B, K), 2)
    kq = K - 1
    for b in range(B):
        valid = np.flatnonzero(mask[b] == 1)
        if not len(valid):
            continue
        regular = np.array([g for g in valid if g not in (g1, g2)] or [g1])
        slot = regular[np.arange(K) % len(regular)]
        cls[b] = rng.permutation(K) % 3
        cls[b, kq] = 0
        slot[kq] = g1
        radius = np.array([0.1, 0.45, 0.9])[cls[b]] * (1 + rng.uniform(-0.1, 0.1, K))
        way = rng.standard_normal((K, 3))
        way /= np.linalg.norm(way, axis=1, keepdims=True)
        agg[b] = c["center_label"][b, slot].astype(np.float64) + radius[:, None] * way
    if no_positive:
        agg += 50.0
    center = agg + rng.normal(0, 0.12, (B, K, 3))
    for b in range(B):
        if mask[b].any():
            at = c["center_label"][b, g1].astype(np.float64)
            off = center[b] - at
            n = np.linalg.norm(off, axis=1, keepdims=True)
            center[b] = np.where(n < 0.05, at + off / np.maximum(n, 1e-9) * 0.05, center[b])  # keep clear of g1
            center[b, kq] = at + (0.01, 0.02, -0.01)
    c["agg_xyz"], c["center"] = f(agg), f(center)
    c["obj"] = f(rng.standard_normal((B, K, 2)) * 2)
    c["h_scores"] = f(rng.standard_normal((B, K, NH)) * 2)
    c["h_resn"] = f(rng.uniform(-0.9, 0.9, (B, K, NH)))
    c["s_scores"] = f(rng.standard_normal((B, K, NS)) * 2)
    c["s_resn"] = f(rng.uniform(-0.4, 0.6, (B, K, NS, 3)))
    c["sem"] = f(rng.standard_normal((B, K, NC)) * 2)
    c["iou"] = f(rng.standard_normal((B, K, NI)) * 2)
    c["iou_jit"] = f(rng.standard_normal((B, K, NI)) * 2)
    c["jitter_center"] = f(center + rng.normal(0, 0.1, (B, K, 3)))
    c["jitter_size"] = f(rng.uniform(0.1, 2.0, (B, K, 3)))
    c["jitter_heading"] = f(rng.uniform(-np.pi, np.pi, (B, K)))

    # ---- planted edges of scene ps
    pos = np.flatnonzero(cls[ps] == 0)
    neg = np.flatnonzero(cls[ps] == 2)
    pa, pb, pc = (int(pos[i % len(pos)]) for i in range(3))
    c["plants"] = dict(kq=kq, g1=g1, g2=g2, pa=pa, pb=pb, pc=pc, scene=ps, empty_scene=empty_scene)
    c["obj"][ps, pa] = (40, -40)
    c["sem"][ps, pa, 0], c["sem"][ps, pa, NC - 1] = 60, -60
    c["h_resn"][ps, pa], c["s_resn"][ps, pa] = 3.0, 2.5
    c["obj"][ps, pb] = (-40, 40)
    c["s_scores"][ps, pb, 0], c["s_scores"][ps, pb, NS - 1] = 60, -60
    c["h_resn"][ps, pb], c["s_resn"][ps, pb] = -3.0, -1.5
    if NH > 1:
        c["h_scores"][ps, pc, 0], c["h_scores"][ps, pc, NH - 1] = -60, 10
        c["h_resn"][ps, pc, NH - 1] = 0.8  # (NH-1) 2pi/NH + 0.8 pi/NH > pi
    if len(neg):
        c["obj"][ps, int(neg[0])] = (-40, 40)
    for key in ("obj", "h_scores", "s_scores", "sem"):
        _separate_top(c[key])
    # a heading that decodes next to pi would make the wrap hang on a rounding: such residuals are moved by
    # 0.05 of a bin's half width (predictions: normalised residuals of every class, labels: radians)
    if NH > 1:
        per, half = 2 * np.pi / NH, np.pi / NH
        angle = np.arange(NH) * per + c["h_resn"].astype(np.float64) * half
        c["h_resn"][np.abs(angle - np.pi) < 1e-3] += F32(0.05)
        angle = c["heading_class_label"] * per + c["heading_residual_label"].astype(np.float64)
        c["heading_residual_label"][np.abs(angle - np.pi) < 1e-3] += F32(0.05 * half)

    # ---- planted IoU labels (the IoU kernel has its own tests)
    rows = 2 * K if jitter else K
    c["iou_lab"] = f(rng.random((B, rows)))
    c["iou_lab"][0, 0], c["iou_lab"][0, 1 % rows], c["iou_lab"][B - 1, rows - 1] = 0.0, 1.0, 1.0
    if rows > 2:
        c["iou_lab"][0, rows // 2] = 0.0
    c["iou_assign"] = rng.integers(0, G, (B, rows)).astype(np.int32)

    # ---- seeds and votes
    c["seed_xyz"] = f(rng.uniform(-4, 4, (B, S, 3)))
    c["seed_inds"] = rng.integers(0, max(N, 1), (B, S)).astype(np.int32)
    c["vote_label"] = f(rng.normal(0, 0.5, (B, N, 9)))
    vmask = rng.integers(0, 2, (B, N)).astype(np.int64)
    if N and S:
        vmask[np.arange(B), c["seed_inds"][:, 0]] = 1  # the first and the last seed are object seeds
        vmask[np.arange(B), c["seed_inds"][:, S - 1]] = 1
    if no_positive:
        vmask[:] = 0
    c["vote_label_mask"] = vmask
    votes = np.zeros((B, S, VF, 3))
    if S:
        gt = np.take_along_axis(c["vote_label"].astype(np.float64), c["seed_inds"].astype(np.int64)[..., None], 1)
        gt = gt.reshape(B, S, 3, 3)
        pick = gt[np.arange(B)[:, None], np.arange(S)[None], np.arange(S)[None] % 3]
        votes = (c["seed_xyz"].astype(np.float64) + pick)[:, :, None] + rng.normal(0, 0.1, (B, S, VF, 3))
        votes[:, :, 1:] += rng.normal(0, 0.5, (B, S, VF - 1, 3))
    c["vote_xyz"] = f(votes.reshape(B, S * VF, 3))

    # ---- no label may hang on a rounding: move offenders by the fixed rule, then assert
    for b in range(B):
        empty = c["center_label"][b][mask[b] != 1]
        assert (empty == empty[:1]).all(), "the empty slots of a scene must be one point"
    for attempt in range(8):
        bad = margins(c)
        if not bad:
            break
        for kind, b, i, other in bad:
            if kind == "agg":
                c["agg_xyz"][b, i] += SHIFT
            elif kind == "center":
                c["center"][b, i] += SHIFT
            elif kind == "gt":
                c["center"][b, other] += SHIFT
            else:
                c["vote_xyz"][b, i * VF:(i + 1) * VF] += SHIFT
    assert not margins(c), margins(c)[:5]
    return c


# ------------------------------------------------------------------ tensors for the binding
def strided3(t):
    """(B, K, C) with the memory of (B, C, K): the transposed slice of a head's output"""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def strided4(t):
    """(B, K, NS, 3) with the memory of (B, NS, 3, K)"""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def tensors(c, dev):
    """name -> torch tensor on dev, head outputs in the case's layout"""
    out = {}
    for key, v in c.items():
        if isinstance(v, np.ndarray):
            t = torch.from_numpy(v.copy()).to(dev)
            if c["layout"] == "strided":
                if key in HEADS3:
                    t = strided3(t)
                elif key == "s_resn":
                    t = strided4(t)
            out[key] = t
    if c["layout"] == "strided":
        assert not out["center"].is_contiguous() or c["K"] == 1
    return out


# ------------------------------------------------------------------ float64 truth
def _huber(x):
    a = x.abs()
    return torch.where(a <= 1, 0.5 * x * x, a - 0.5)


def _first_argmin(d, dim):
    """numpy's rule: the FIRST minimum"""
    return torch.from_numpy(np.argmin(d.detach().numpy(), axis=dim))


def _class2angle(cls, res, nh):
    """config.class2angle_gpu with its fp32 constants, in float64; also the magnitude the bound scales with"""
    if nh == 1:
        return np.zeros(cls.shape), np.zeros(cls.shape)
    base = cls.astype(np.float64) * np.float64(F32(2 * np.pi / nh))
    angle = base + res
    wrap = angle > np.float64(F32(np.pi))
    assert (np.abs(angle - np.pi) > 1e-4).all(), "a heading decodes next to pi"
    return angle - wrap * np.float64(F32(2 * np.pi)), base + np.abs(res) + np.float64(F32(2 * np.pi))


def decode_reference(c):
    """boxes (B, rows, 7), gt_boxes (B, G, 7) in float64 and their bounds: one fp32 rounding per operation
    the kernel performs (loss_core.h decode_prediction / decode_ground_truth).
      prediction: centre copied (0); size = mean + resn * mean (2), exactly float32(1e-6) where <= 0;
                  heading = -(cls * per + resn * (pi/NH) [- 2 pi]) (product, product, sum, wrap: 4)
      GT:         centre copied or -1000 (0); size = mean + residual (1); heading (product, sum, wrap: 3)
      jittered:   copies (0)"""
    d = np.float64
    B, K, G, NH = c["B"], c["K"], c["G"], c["NH"]
    mean = c["mean_size"].astype(d)
    hc, sc = np.argmax(c["h_scores"], -1), np.argmax(c["s_scores"], -1)
    resn = np.take_along_axis(c["s_resn"].astype(d), sc[..., None, None], 2)[:, :, 0]
    size = mean[sc] + resn * mean[sc]
    assert (np.abs(size) > 1e-5).all(), "a decoded size next to 0"
    size_bound = 2 * EPS * (np.abs(mean[sc]) + np.abs(resn * mean[sc]))
    clamped = size <= 0
    size, size_bound = np.where(clamped, d(F32(1e-6)), size), np.where(clamped, 0.0, size_bound)
    h_res = np.take_along_axis(c["h_resn"].astype(d), hc[..., None], 2)[..., 0] * d(F32(np.pi / NH))
    angle, scale = _class2angle(hc, h_res, NH)
    boxes = np.concatenate([c["center"].astype(d), size, -angle[..., None]], -1)
    bound = np.concatenate([np.zeros((B, K, 3)), size_bound, (4 * EPS * scale)[..., None]], -1)
    if c["jitter"]:
        jit = np.concatenate([c["jitter_center"], c["jitter_size"], -c["jitter_heading"][..., None]], -1).astype(d)
        boxes, bound = np.concatenate([boxes, jit], 1), np.concatenate([bound, np.zeros((B, K, 7))], 1)
    empty = (c["box_label_mask"] != 1)[..., None]
    gsc = c["size_class_label"]
    gsize = mean[gsc] + c["size_residual_label"].astype(d)
    gangle, gscale = _class2angle(c["heading_class_label"], c["heading_residual_label"].astype(d), NH)
    gt = np.concatenate([np.where(empty, -1000.0, c["center_label"].astype(d)), gsize, -gangle[..., None]], -1)
    gt_bound = np.concatenate([np.zeros((B, G, 3)), EPS * (np.abs(mean[gsc]) + np.abs(c["size_residual_label"])),
                               (3 * EPS * gscale)[..., None]], -1)
    return dict(boxes=boxes, boxes_bound=bound, gt_boxes=gt, gt_boxes_bound=gt_bound, clamped=clamped)


@functools.lru_cache(maxsize=None)
def reference(name, consistency=False, no_positive=False, grad_scale=1.0):
    """float64 labels, statistics (name -> float) and gradients of grad_scale * loss (name of _GRADS ->
    numpy array) of a case; computed once and shared (read-only)."""
    c = build(name, consistency, no_positive)
    B, K, G, S, VF, NH = c["B"], c["K"], c["G"], c["S"], c["VF"], c["NH"]
    d = torch.float64
    t = {k: torch.from_numpy(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    leaf = {k: t[k].to(d).requires_grad_(True) for k in GRAD_OF.values()}
    f = lambda k: t[k].to(d)  # noqa: E731
    gather = lambda v, idx: torch.gather(v, 1, idx)  # noqa: E731
    total = float(B * K)
    st = {}

    # objectness: distance of the aggregated vote to the nearest non-empty GT centre
    valid = (t["box_label_mask"] == 1)
    masked = torch.where(valid[..., None], f("center_label"), torch.full((), -1000.0, dtype=d))
    d2 = ((f("agg_xyz")[:, :, None] - masked[:, None]) ** 2).sum(-1)      # (B, K, G)
    assign = _first_argmin(d2, 2)
    dist = torch.sqrt(torch.gather(d2, 2, assign[..., None])[..., 0] + 1e-6)
    label = dist < NEAR
    omask = ((dist < NEAR) | (dist > FAR)).to(d)
    obj = label.to(d)
    cnt, msum = obj.sum(), omask.sum()
    w = torch.where(label, 0.8, 0.2).to(d)
    lse = torch.logsumexp(leaf["obj"], -1)
    ce = w * (lse - torch.gather(leaf["obj"], 2, label.long()[..., None])[..., 0])
    st["objectness_loss"] = (ce * omask).sum() / (msum + 1e-6)
    st["obj_acc"] = (((leaf["obj"][..., 1] > leaf["obj"][..., 0]) == label).to(d) * omask).sum() / (msum + 1e-6)
    st["pos_ratio"] = cnt / total
    st["neg_ratio"] = msum / total - st["pos_ratio"]
    st["obj_count"] = cnt
    pos_mean = lambda v: (v * obj).sum() / (cnt + 1e-6)  # noqa: E731

    # centre: chamfer between predicted centres and the RAW centre labels
    dc = ((leaf["center"][:, :, None] - f("center_label")[:, None]) ** 2).sum(-1)  # (B, K, G)
    near_c = _first_argmin(dc, 2)
    gt_nearest = _first_argmin(dc, 1)                                               # (B, G)
    center1 = torch.gather(dc, 2, near_c[..., None])[..., 0]
    dist2 = torch.gather(dc, 1, gt_nearest[:, None])[:, 0]
    bmask = f("box_label_mask")
    st["center_loss"] = pos_mean(center1) + (dist2 * bmask).sum() / (bmask.sum() + 1e-6)

    def cross_entropy(scores, cls):
        return torch.logsumexp(scores, -1) - torch.gather(scores, 2, cls[..., None])[..., 0]

    hl = gather(t["heading_class_label"], assign)
    st["heading_cls_loss"] = pos_mean(cross_entropy(leaf["h_scores"], hl))
    target = gather(f("heading_residual_label"), assign) / (np.pi / NH)
    st["heading_reg_loss"] = pos_mean(_huber(torch.gather(leaf["h_resn"], 2, hl[..., None])[..., 0] - target))
    sl = gather(t["size_class_label"], assign)
    st["size_cls_loss"] = pos_mean(cross_entropy(leaf["s_scores"], sl))
    s_target = torch.gather(f("size_residual_label"), 1, assign[..., None].expand(-1, -1, 3)) / f("mean_size")[sl]
    s_pred = torch.gather(leaf["s_resn"], 2, sl[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
    st["size_reg_loss"] = pos_mean(_huber(s_pred - s_target).mean(-1))
    cl = gather(t["sem_cls_label"], assign)
    st["sem_cls_loss"] = pos_mean(cross_entropy(leaf["sem"], cl))
    st["cls_acc"] = pos_mean((torch.from_numpy(np.argmax(c["sem"], -1)) == cl).to(d))
    st["box_loss"] = (0.1 * st["heading_cls_loss"] + st["heading_reg_loss"] + 0.1 * st["size_cls_loss"]
                      + st["size_reg_loss"] + st["center_loss"])

    if consistency:
        st["loss"] = 10 * (st["box_loss"] + 0.1 * st["sem_cls_loss"])
        st["vote_loss"] = st["iou_loss"] = st["jitter_iou_loss"] = torch.zeros((), dtype=d)
    else:
        def iou_term(scores, lab, who):
            p = torch.sigmoid(scores)
            if p.shape[2] > 1:
                p = torch.gather(p, 2, gather(t["sem_cls_label"], who.long())[..., None])
            return p[..., 0] - lab

        lab, who = f("iou_lab"), t["iou_assign"]
        x = iou_term(leaf["iou"], lab[:, :K], who[:, :K])
        st["iou_loss"] = _huber(x).mean()
        st["iou_acc"] = x.abs().mean()
        st["iou_acc_obj"] = pos_mean(x.abs())
        st["pred_iou_value"] = lab[:, :K].mean()
        st["pred_iou_obj_value"] = pos_mean(lab[:, :K])
        st["jitter_iou_loss"] = torch.zeros((), dtype=d)
        if c["jitter"]:
            xj = iou_term(leaf["iou_jit"], lab[:, K:], who[:, K:])
            st["jitter_iou_loss"] = _huber(xj).sum() / (total + 1e-6)
            st["jitter_iou_acc"] = xj.abs().mean()
            st["jitter_iou_acc_obj"] = xj.abs().sum() / (total + 1e-6)
        # votes: the closest (vote, GT vote) pair of every seed, L1, averaged over the object seeds
        inds = t["seed_inds"].long()
        vmask = gather(t["vote_label_mask"], inds).to(d)
        gt = torch.gather(f("vote_label"), 1, inds[..., None].expand(-1, -1, 9)).view(B, S, 1, 3, 3)
        gt = gt + f("seed_xyz").view(B, S, 1, 1, 3)
        pair = (leaf["vote_xyz"].view(B, S, VF, 1, 3) - gt).abs().sum(-1).reshape(B, S, VF * 3)
        best = torch.gather(pair, 2, _first_argmin(pair, 2)[..., None])[..., 0]
        st["vote_loss"] = (best * vmask).sum() / (vmask.sum() + 1e-6)
        st["loss"] = 10 * (st["vote_loss"] + 0.5 * st["objectness_loss"] + st["box_loss"]
                           + 0.1 * st["sem_cls_loss"] + st["iou_loss"] + st["jitter_iou_loss"])

    (st["loss"] * grad_scale).backward()
    grads = {}
    for g, key in GRAD_OF.items():
        v = leaf[key].grad
        grads[g] = (torch.zeros_like(leaf[key]) if v is None else v).numpy()
    return dict(stats={k: float(v.detach()) for k, v in st.items()}, grads=grads,
                objectness_label=label.long().numpy(), objectness_mask=omask.numpy(),
                object_assignment=assign.numpy(), gt_nearest=gt_nearest.numpy(), **decode_reference(c))
