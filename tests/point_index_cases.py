"""Cases the CPU and the GPU tests of the point index share (test_point_index.py,
test_point_index_gpu.py): key planes over one or several scans, every array from a fixed seed.  A case is
{cap, count (S,) int32, offset (S,) int64, keys (P,) int32}; its scans tile the key plane.  The host
results (`want`) are computed once per case and shared: do not write to them.

  len<n>       one scan of n rows, n over the wave (64), tile (INDEX_TILE) and segment (INDEX_SEGMENT) edges
               and 2 segments + 3 (the cursor carried across segments); random keys, 30 % unowned.
  patterns, all at n = 2 * INDEX_SEGMENT + 3:
    one_key      one key for all, a long run
    distinct64   64 distinct keys in every wave
    alternate    two keys alternating: the stability probe across every boundary
    all_unowned  all -1
    random30     random with 30 % -1
    out_of_range keys >= cap and < -1 mixed in: they go to the tail
  three        S = 3 with unequal counts, scan 1 all -1
  empty_between  a scan with count = 0 between two others (launch level: a ScanStore has no empty scan)
  cap1, cap8191 (the last one-pass value: the tail shares the top digit), cap8192, cap8197 (two passes:
               keys that differ only in the high digit, keys that differ only in the low one)
"""
import importlib

import numpy as np

from conftest import load_pkg

load_pkg()
PI = importlib.import_module("3dioumatch_amd.votenet.point_index")

SEG, TILE, BITS = PI.INDEX_SEGMENT, PI.INDEX_TILE, PI.INDEX_DIGIT_BITS
DIGITS = 1 << BITS
LONG = 2 * SEG + 3
LENGTHS = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, SEG - 1, SEG, SEG + 1, LONG)
LENGTH_CAP = 37
PATTERN_CAP = 100
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def random_keys(n, cap, seed, unowned=0.3, bad=()):
    """(n,) int32: uniform over 0..cap-1, a share `unowned` of -1, and with `bad` a tenth of the rows
    drawn from those out-of-range values"""
    g = np.random.default_rng(seed)
    keys = g.integers(0, cap, n).astype(np.int64)
    keys[g.random(n) < unowned] = -1
    if len(bad):
        hit = g.random(n) < 0.1
        keys[hit] = g.choice(np.asarray(bad, np.int64), int(hit.sum()))
    return keys.astype(np.int32)


def _case(cap, parts):
    count = np.array([len(p) for p in parts], np.int32)
    offset = np.concatenate([[0], np.cumsum(count[:-1], dtype=np.int64)]).astype(np.int64)
    keys = np.concatenate(parts).astype(np.int32) if int(count.sum()) else np.zeros(0, np.int32)
    return {"cap": int(cap), "count": count, "offset": offset, "keys": keys}


def _digit_edge(cap, n, seed):
    """keys around the digit boundary of `cap`: k and k + 2^BITS where both are below cap (they differ
    only in the high digit; with cap = 2^BITS the partner is the tail bucket), runs of neighbouring low
    values (they differ only in the low digit), the largest keys, -1 and out-of-range ones"""
    g = np.random.default_rng(seed)
    low = np.arange(0, 5)
    pool = [low, low + DIGITS, np.array([DIGITS - 2, DIGITS - 1, cap - 2, cap - 1, cap, cap + 1, -1, -1, -1]),
            g.integers(0, cap, 40)]
    pool = np.concatenate(pool).astype(np.int64)
    return g.choice(pool, n).astype(np.int32)


def _build():
    c = {}
    for i, n in enumerate(LENGTHS):
        c["len%d" % n] = _case(LENGTH_CAP, [random_keys(n, LENGTH_CAP, 100 + i)])
    j = np.arange(LONG)
    c["one_key"] = _case(PATTERN_CAP, [np.full(LONG, 5)])
    c["distinct64"] = _case(PATTERN_CAP, [(j * 37 + j // 64) % 64])  # a permutation of 0..63 in every wave of 64
    c["alternate"] = _case(PATTERN_CAP, [np.where(j % 2 == 0, 7, 2)])
    c["all_unowned"] = _case(PATTERN_CAP, [np.full(LONG, -1)])
    c["random30"] = _case(PATTERN_CAP, [random_keys(LONG, PATTERN_CAP, 201)])
    c["out_of_range"] = _case(PATTERN_CAP, [random_keys(LONG, PATTERN_CAP, 202, bad=(
        PATTERN_CAP, PATTERN_CAP + 1, DIGITS, DIGITS + 3, INT_MAX, -2, -3, -DIGITS, INT_MIN))])
    c["three"] = _case(50, [random_keys(SEG + 5, 50, 301), np.full(300, -1), random_keys(2 * SEG + 1, 50, 302)])
    c["empty_between"] = _case(20, [random_keys(500, 20, 311), np.zeros(0, np.int32), random_keys(700, 20, 312)])
    c["cap1"] = _case(1, [random_keys(1000, 1, 401, unowned=0.5, bad=(1, 2, -2))])
    c["cap8191"] = _case(DIGITS - 1, [_digit_edge(DIGITS - 1, 3000, 402)])
    c["cap8192"] = _case(DIGITS, [_digit_edge(DIGITS, 3000, 403), _digit_edge(DIGITS, 700, 404)])
    c["cap8197"] = _case(DIGITS + 5, [_digit_edge(DIGITS + 5, SEG + 77, 405)])
    for case in c.values():
        for a in case.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


CASES = _build()
LENGTH_CASES = ["len%d" % n for n in LENGTHS]
PATTERN_CASES = ["one_key", "distinct64", "alternate", "all_unowned", "random30", "out_of_range"]
SCAN_CASES = ["three", "empty_between"]
DIGIT_CASES = ["cap1", "cap8191", "cap8192", "cap8197"]
assert sorted(CASES) == sorted(LENGTH_CASES + PATTERN_CASES + SCAN_CASES + DIGIT_CASES)
assert all((np.sort(CASES["distinct64"]["keys"][w:w + 64]) == np.arange(64)).all() for w in range(0, LONG - 63, 64))
assert PI.passes_of(CASES["cap8191"]["cap"]) == 1 and PI.passes_of(CASES["cap8192"]["cap"]) == 2

_want = {}


def get(case):
    """The case (shared: do not write to it)."""
    return CASES[case]


def buckets(case, s):
    """(n,) int64: the bucket of every row of scan s, by the rule's own words"""
    c = CASES[case]
    k = c["keys"][int(c["offset"][s]):int(c["offset"][s]) + int(c["count"][s])].astype(np.int64)
    return np.where((k >= 0) & (k < c["cap"]), k, c["cap"])


def want(case):
    """host_point_index of the case, computed once."""
    if case not in _want:
        c = CASES[case]
        got = PI.host_point_index(c["keys"], c["offset"], c["count"], c["cap"])
        for a in got.values():
            a.setflags(write=False)
        _want[case] = got
    return _want[case]
