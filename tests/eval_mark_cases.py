"""Inputs and a plain reference for the tests of the AP marking (eval_det._mark on the host,
csrc/eval_ap.hip eval_mark_kernel on the device); no package import.

  loop_mark(ovmax, gt_id, npos, thr)   the reference's marking of ONE class as it reads
                      (utils/eval_det.py:119-157 and the non-07 branch of voc_ap, :46-60): a walk over
                      the detections in the given order with a set of claimed ground-truth ids, cumsum,
                      the padded envelope looped from the right, the sum over the positions where the
                      recall changes.  No np.unique, no vectorised envelope: independent of
                      eval_det._mark.  The sum is math.fsum (exactly rounded), so its own error is one
                      rounding.
  mark_case(seed)     11 class segments on both sides of the kernel's 256-detection chunk (and empty
                      ones), with repeat claims, threshold-equal IoUs and -inf entries.
  envelope_case()     one class of 773 detections whose precision peaks in its fourth chunk: the envelope of
                      the first chunk's true positives comes from three chunks later.
  reference(seed, thr)  loop_mark of every segment of mark_case(seed), computed once and shared.
  cross_chunk_claims / raised_chunks   what the builder's own test counts.
"""
import functools
import math

import numpy as np

CHUNK = 256                     # eval_ap.hip kMarkThreads
LENGTHS = (0, 1, 255, 256, 257, 513, 1000, 0, 300, 2049, 1000)
NPOS = (3, 1, 40, 40, 40, 600, 150, 0, 0, 64, 50)
ALL_INF, REVERSED = 8, 10       # the segment without ground truth; the one whose hits are all in its last chunk
REVERSED_FROM = 768             # the reversed segment's first rank that may hit
SPARE_IDS = 5                   # ground-truth ids that no class owns


def loop_mark(ovmax, gt_id, npos, thr):
    """-> rec (n) f64, prec (n) f64, ap (Python float); detections are in rank order."""
    n = len(ovmax)
    tp, fp = np.zeros(n), np.zeros(n)
    claimed = set()
    for d in range(n):
        if float(ovmax[d]) > thr:
            j = int(gt_id[d])
            if j not in claimed:
                tp[d] = 1.
                claimed.add(j)
            else:
                fp[d] = 1.
        else:
            fp[d] = 1.
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    with np.errstate(invalid="ignore", divide="ignore"):
        rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    mrec = [0.] + [float(v) for v in rec] + [1.]
    mpre = [0.] + [float(v) for v in prec] + [0.]
    for i in range(len(mpre) - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i])
    terms = [(mrec[i] - mrec[i - 1]) * mpre[i] for i in range(1, len(mrec)) if mrec[i] != mrec[i - 1]]
    return rec, prec, math.fsum(terms)


@functools.lru_cache(maxsize=None)
def mark_case(seed):
    """-> dict(seg (C+1) i64, ovmax (n) f64, gt_id (n) i32, npos (C) i64, num_gt); read-only, shared.

    Class c owns the ground-truth ids [base_c, base_c + npos_c).  Within a segment of length L:
    ovmax = clip(1.2 U(0,1) - 0.6 rank / L, 0, 1) (IoU falls with the rank on average, as in a
    score-ordered list), then about 10 % of the entries are -inf, about 3 % exactly 0.25 and about 3 %
    exactly 0.5 (the strict `>` rejects these at their threshold).  gt_id is uniform over the class's
    own ids; a -inf entry has id 0, another class's, which is what the calculator stores for an
    unmatched slot.  The segment without ground truth is all -inf; the last segment is -inf below rank
    768, so that the envelope of every chunk but its last is only what the later chunks carry in."""
    rng = np.random.default_rng([seed, 256])
    npos = np.array(NPOS, np.int64)
    base = np.concatenate([[0], np.cumsum(npos)])
    seg = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    ovmax, gt_id = np.zeros(seg[-1]), np.zeros(seg[-1], np.int32)
    for c, (length, p) in enumerate(zip(LENGTHS, NPOS)):
        if length == 0:
            continue
        rank = np.arange(length)
        ov = np.clip(1.2 * rng.random(length) - 0.6 * rank / length, 0.0, 1.0)
        kind = rng.random(length)
        ov[kind < 0.10] = -np.inf
        ov[(kind >= 0.10) & (kind < 0.13)] = 0.25
        ov[(kind >= 0.13) & (kind < 0.16)] = 0.5
        gid = base[c] + rng.integers(0, max(p, 1), length)
        if c == ALL_INF or p == 0:
            ov[:] = -np.inf
        if c == REVERSED:
            ov[:REVERSED_FROM] = -np.inf
        gid[np.isneginf(ov)] = 0
        ovmax[seg[c]:seg[c + 1]], gt_id[seg[c]:seg[c + 1]] = ov, gid
    for a in (seg, ovmax, gt_id, npos):
        a.setflags(write=False)
    return dict(seg=seg, ovmax=ovmax, gt_id=gt_id, npos=npos, num_gt=int(npos.sum()) + SPARE_IDS)


@functools.lru_cache(maxsize=None)
def envelope_case():
    """mark_case's dict for ONE class of 3 * 256 + 5 detections and 300 boxes, every hit a box of its own.
    In mark_case the recall of a long segment changes where the precision is already falling, or (the
    reversed segment) only in the last chunk, so the AP seldom depends on an envelope carried further than
    one chunk.  Here ranks 8, 24, .. 248 and 300 hit, the rest of the first two chunks misses, and every
    rank from 512 on hits: the precision is about 0.06 at rank 255, 0.03 at rank 511, 273 / 768 at rank 767
    and 278 / 773, its maximum, at the last rank -- what the terms of the first chunk are multiplied by."""
    n = 3 * CHUNK + 5
    ovmax = np.full(n, -np.inf)
    hit = np.concatenate([np.arange(8, CHUNK, 16), [300], np.arange(2 * CHUNK, n)])
    ovmax[hit] = 0.75
    gt_id = np.zeros(n, np.int32)
    gt_id[hit] = np.arange(len(hit))
    return dict(seg=np.array([0, n], np.int64), ovmax=ovmax, gt_id=gt_id, npos=np.array([300], np.int64),
                num_gt=300)


def segment(case, c):
    """-> ovmax, gt_id, npos of class c"""
    s0, s1 = int(case["seg"][c]), int(case["seg"][c + 1])
    return case["ovmax"][s0:s1], case["gt_id"][s0:s1], int(case["npos"][c])


@functools.lru_cache(maxsize=None)
def reference(seed, thr):
    """-> per class (rec, prec, ap) of loop_mark, None for an empty segment; read-only, shared."""
    case = mark_case(seed)
    out = []
    for c in range(len(LENGTHS)):
        ov, gid, npos = segment(case, c)
        out.append(loop_mark(ov, gid, npos, thr) if len(ov) else None)
    return out


def permuted_ids(case, seed=7):
    """gt_id with every class's own id range permuted by a fixed bijection; id 0 of the -inf entries
    stays (it is no id of the entry's class)."""
    rng = np.random.default_rng(seed)
    base = np.concatenate([[0], np.cumsum(case["npos"])])
    out = case["gt_id"].copy()
    for c in range(len(LENGTHS)):
        s0, s1 = int(case["seg"][c]), int(case["seg"][c + 1])
        p = int(case["npos"][c])
        if s1 == s0 or p == 0:
            continue
        perm = base[c] + rng.permutation(p)
        own = np.isfinite(case["ovmax"][s0:s1])
        out[s0:s1][own] = perm[case["gt_id"][s0:s1][own] - base[c]]
    return out


def cross_chunk_claims(ovmax, gt_id, thr):
    """detections above thr whose ground-truth id was first claimed in an EARLIER chunk"""
    first, count = {}, 0
    for d in range(len(ovmax)):
        if float(ovmax[d]) > thr:
            j = int(gt_id[d])
            if j not in first:
                first[j] = d
            elif first[j] // CHUNK < d // CHUNK:
                count += 1
    return count


def raised_chunks(prec):
    """chunks whose envelope a later chunk raises: max(prec[later chunks]) > min(prec[chunk])"""
    n = len(prec)
    return [k for k in range((n - 1) // CHUNK)
            if prec[(k + 1) * CHUNK:].max() > prec[k * CHUNK:(k + 1) * CHUNK].min()]
