"""Cases the CPU and the GPU tests of the mask matching share (test_mask_eval.py, test_mask_eval_gpu.py).
A case is a set of packed detections in label_points_cases' form (its `planes`, `arena` and `found`
build the Detections: the case is placed in that module's cache of built cases under a `mask_` name),
per-point owners as label_points would leave them (a PointLabels built from its word buffer) and
per-point truth.  Every array comes from a fixed seed; `want` is host_match_masks of the case, computed
once and shared: do not write to it.

  lengths   scans of 1, B - 1, B, B + 1 and 3 B + 1 points (B = MASK_BLOCK), cap = 8
  empty     S = 3 scans of 300, 0 and 77 points: an empty scan between two others
  g1, g63, g64, g65   G on both sides of the match wave's stride
  waves     one scan of 5 B points laid out wave by wave: a wave of one key, a wave of 64 distinct
            (r, g) keys, 64 distinct g under one r, one g under 64 distinct r, a run across a wave and a
            workgroup boundary, unset lanes interleaved with set ones, a wave whose last lane alone is set,
            waves of six runs (two more than the merge's rounds) and waves of five scattered keys
  scores    per-class scores (NS = 18) with a class out of range among the rows
  noisy0, noisy1   masks that are noisy copies of the truth instances: partial AP, ties in score
"""
import importlib

import numpy as np

import label_points_cases as cases
from conftest import load_pkg

load_pkg()
PL = importlib.import_module("3dioumatch_amd.votenet.point_labels")
ME = importlib.import_module("3dioumatch_amd.votenet.mask_eval")

F = np.float32
B = ME.MASK_BLOCK
NUM_CLASS = 18
G_VALUES = (1, 63, 64, 65)


def register(name, owners, truth_instance, truth_class, count, cls, score, cap):
    """Place the case in label_points_cases' cache and return its name there.  `owners`,
    `truth_instance`, `truth_class`: one array per scan; count (S,), cls (S, cap), score (S, cap) or
    (S, cap, NS)."""
    S = len(owners)
    score = np.asarray(score, F)
    NS = score.shape[2] if score.ndim == 3 else 0
    planes = {"count": np.asarray(count, np.int32), "cls": np.asarray(cls, np.int32), "score": score,
              "box": np.zeros((S, cap, 7), F)}
    key = "mask_" + name
    c = {"layout": "plain", "K": cap, "cap": cap, "NC": NS, "planes": planes,
         "clouds": [np.zeros((len(o), 3), F) for o in owners], "names": ["%s_%d" % (key, s) for s in range(S)],
         "owners": [np.asarray(o, np.int32) for o in owners],
         "truth_instance": [np.asarray(t, np.int32) for t in truth_instance],
         "truth_class": [np.asarray(t, np.int32) for t in truth_class]}
    for a in list(planes.values()) + c["owners"] + c["truth_instance"] + c["truth_class"]:
        a.setflags(write=False)
    cases._cases[key] = c
    return key


def random_case(name, lengths, cap, G, seed, NS=0):
    g = np.random.default_rng(seed)
    S = len(lengths)
    klass_of = g.integers(-1, NUM_CLASS + 1, (S, G))  # -1 and NUM_CLASS: not a class
    klass_of[:, 0] = 3  # row 0 of scan 0 is of this class: at least one match, also with G = 1
    owners, ti, tc = [], [], []
    for s, n in enumerate(lengths):
        run = np.sort(g.integers(0, G + 1, n))  # coherent: runs of one instance, 0 = none
        t = np.where(g.random(n) < 0.8, run, g.integers(0, G + 1, n))
        o = np.where(g.random(n) < 0.7, (t + g.integers(0, 2, n)) % (cap + 1) - 1, g.integers(-1, cap, n))
        owners.append(o)
        ti.append(t)
        k = klass_of[s][np.maximum(t, 1) - 1]
        tc.append(np.where(g.random(n) < 0.05, g.integers(-2, NUM_CLASS + 2, n), k))  # some instances of mixed class
    count = g.integers(0, cap + 1, S)
    count[0] = cap
    cls = g.integers(-1, NUM_CLASS + 1, (S, cap))
    cls[0, 0] = 3
    score = (g.integers(0, 6, (S, cap, NS) if NS else (S, cap)) / F(5)).astype(F)  # ties
    return register(name, owners, ti, tc, count, cls, score, cap)


def waves_case():
    n, cap, G = 5 * B, 80, 70
    o, t = np.full(n, -1), np.zeros(n, np.int64)
    lane = np.arange(64)
    o[0:64], t[0:64] = 3, 6                                  # wave 0: one key
    o[64:128], t[64:128] = lane, lane + 1                    # wave 1: 64 distinct (r, g)
    o[128:192], t[128:192] = 7, lane + 1                     # wave 2: one r, 64 distinct g
    o[192:256], t[192:256] = lane, 9                         # wave 3: 64 distinct r, one g
    o[B - 40:B + 90], t[B - 40:B + 90] = 2, 2                # a run over the ends of wave 3, workgroup 0 and wave 4
    w = 2 * B                                                # wave 8: unset lanes among set ones
    o[w:w + 64] = np.where(lane % 2 == 0, 5, -1)
    t[w:w + 64] = np.where(lane % 3 == 0, 0, 11 + lane % 2)
    o[w + 127], t[w + 127] = 1, 70                           # wave 9: the last lane alone, and the last g
    w = 3 * B                                                # waves 12, 13: six runs of 11 lanes, two more than the rounds
    o[w:w + 128], t[w:w + 128] = np.arange(128) % 64 // 11, 20 + np.arange(128) % 64 // 11
    o[w + 128:w + 256] = np.arange(128) % 5                  # waves 14, 15: five scattered keys, no runs
    t[w + 128:w + 256] = 20 + np.arange(128) % 5
    w = 4 * B                                                # the last workgroup: g set, r unset, and the reverse
    o[w:w + 128], t[w:w + 128] = -1, 30 + np.arange(128) % 7
    o[w + 128:w + 256], t[w + 128:w + 256] = np.arange(128) % 9, 0
    klass = np.arange(G + 1) % NUM_CLASS
    tc = klass[t]
    tc[64] = -5                                              # g = 0's lowest-index point: of no class
    cls = (np.arange(cap) % NUM_CLASS)[None, :]
    score = ((np.arange(cap) * 7 % 11) / F(11)).astype(F)[None, :]
    return register("waves", [o], [t], [tc], [cap], cls, score, cap)


def noisy_case(name, seed, S=3, n=4000, G=12, cap=16):
    """Truth instances are runs of points; row r copies instance r % G with some of its points
    dropped and some foreign ones added, rows >= G duplicate at a lower score."""
    g = np.random.default_rng(seed)
    owners, ti, tc = [], [], []
    klass_of = g.integers(0, 4, (S, G))
    klass_of[:, 0] = -1  # an instance of no class
    cls = np.zeros((S, cap), np.int64)
    for s in range(S):
        t = np.sort(g.integers(0, G + 1, n))
        o = np.where(t > 0, t - 1, -1)
        dup = g.random(n) < 0.25
        o = np.where(dup & (o >= 0) & (o + G < cap), o + G, o)          # a duplicate takes a quarter
        o = np.where(g.random(n) < 0.3 * g.random(), -1, o)             # dropped points
        o = np.where(g.random(n) < 0.1, g.integers(-1, cap, n), o)      # foreign points
        owners.append(o)
        ti.append(t)
        tc.append(klass_of[s][np.maximum(t, 1) - 1])
        cls[s] = klass_of[s][np.arange(cap) % G]
        cls[s, g.integers(0, cap)] = 5                                  # a class without truth
    score = (g.integers(1, 8, (S, cap)) / F(8)).astype(F)
    return register(name, owners, ti, tc, np.full(S, cap), cls, score, cap)


BUILDERS = {
    "lengths": lambda: random_case("lengths", (1, B - 1, B, B + 1, 3 * B + 1), 8, 9, 81),
    "empty": lambda: random_case("empty", (300, 0, 77), 8, 5, 82),
    "waves": waves_case,
    "scores": lambda: random_case("scores", (500, 300), 12, 10, 83, NS=NUM_CLASS),
    "noisy0": lambda: noisy_case("noisy0", 91),
    "noisy1": lambda: noisy_case("noisy1", 92, S=2, n=3000, G=9),
}
BUILDERS.update({"g%d" % G: (lambda G=G: random_case("g%d" % G, (700, 150), 8, G, 84 + G)) for G in G_VALUES})
NAMES = sorted(BUILDERS)
_keys, _want = {}, {}


def key(name):
    """The case's name in label_points_cases' cache (built on first use)."""
    if name not in _keys:
        _keys[name] = BUILDERS[name]()
    return _keys[name]


def get(name):
    return cases.get(key(name))


def truth(name, device=None):
    c = get(name)
    return ME.PointTruth(c["names"], c["truth_instance"], c["truth_class"], device)


def found(name, device=None):
    import torch
    a = cases.arena(key(name))
    return cases.found(key(name), a if device is None else torch.from_numpy(a).to(device), NUM_CLASS)


def labels(name, device=None):
    """The PointLabels label_points would return had it found the case's owners."""
    import torch
    c = get(name)
    count = np.array([len(o) for o in c["owners"]], np.int32)
    offset = np.concatenate([[0], np.cumsum(count, dtype=np.int64)[:-1]]).astype(np.int64)
    instance = np.concatenate(c["owners"]).astype(np.int32)
    points = np.stack([np.bincount(o[o >= 0], minlength=c["cap"]) for o in c["owners"]]).astype(np.int32)
    words = np.concatenate([c["planes"]["count"], points.reshape(-1), instance, np.full(len(instance), -1, np.int32)])
    words = words.astype(np.int32)
    if device is not None:
        words = torch.from_numpy(words).to(device)
    return PL.PointLabels(c["names"], count, offset, c["cap"], "score", 0.0, words, None)


def want(name, min_points=1, min_truth_points=1):
    """host_match_masks of the case, computed once."""
    k = (name, min_points, min_truth_points)
    if k not in _want:
        lab = labels(name)
        got = ME.host_match_masks(lab.instance, lab.points, cases.planes(key(name)), truth(name), NUM_CLASS, min_points,
                                  min_truth_points)
        for a in got.values():
            a.setflags(write=False)
        _want[k] = got
    return _want[k]
