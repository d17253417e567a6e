"""Per-detection point lists, on the device: the points of each detected object, as CSR lists.

    labels = label_points(found, raw)
    index = labels.index()                      # PointIndex: built once, no host read
    index.start, index.order                    # device tensors; index[i], by_name, points_of, lists, owned read
    index.points_of(0, 7)                       # the rows of scan 0 that packed row 7 owns, ascending
    crops = index.gather(raw.dev["cloud"])      # (P, C): every object's points contiguous

label_points colours the points; this turns the colouring into objects.  The primitive is a stable
multi-split of each scan's rows by an integer key (include/point_index_hip.h, csrc/point_index.hip).

The rule.  For each scan s with n = count[s] rows:
  key       k_j of local row j; for labels it is instance[offset[s] + j].
  cap       the number of rows per scan of the detections.
  bucket    b_j = k_j if 0 <= k_j < cap, else cap: the tail is -1 and any out-of-range key.  A bad key
            owns nothing and is never followed as an index.
  order     int32; order[offset[s] : offset[s] + n] is the permutation of 0..n-1 equal to
            np.argsort(b, kind="stable"): row 0's points in ascending index, then row 1's, ..., the
            unowned points last, in ascending index.
  start     (S, cap + 1) int32; start[s, r] = #{j : b_j < r}.  Row r's list is
            order[offset[s] + start[s, r] : offset[s] + start[s, r + 1]]; start[s, cap] is the scan's
            owned total.
Scans never interact; everything is an integer, so two runs are bit-equal.  For keys that came from
label_points, start[s, r + 1] - start[s, r] == points[s, r].

On the device: scene_points_index, an LSD radix split with one digit of INDEX_DIGIT_BITS bits per pass
(cap <= 8191: one pass of four launches; up to INDEX_MAX_CAP, past SCAN_TILE_MAX x SCAN_MAX_K: two).  Nothing in PointLabels.index() copies to the host or
synchronises; the first read of the result makes ONE copy.  `host_point_index` restates the rule in
numpy -- one stable argsort and one bincount per scan -- and is the path of a `device=None` store.
"""
import numpy as np
import torch

from .. import records

INDEX_DIGIT_BITS = 13  # include/point_index_hip.h
INDEX_SEGMENT = 4096   # include/point_index_hip.h
INDEX_TILE = 256       # include/point_index_hip.h
INDEX_MAX_CAP = (1 << (2 * INDEX_DIGIT_BITS)) - 1  # include/point_index_hip.h: two digits


def _cap(cap):
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 1 or cap >= 1 << 31:
        raise ValueError("cap must be an integer in 1..2^31 - 1, got %r" % (cap,))
    return int(cap)


def _device_cap(cap):
    cap = _cap(cap)
    if cap > INDEX_MAX_CAP:
        raise ValueError("cap %d: the device index takes 1..%d (two digits)" % (cap, INDEX_MAX_CAP))
    return cap


def passes_of(cap):
    """radix passes of scene_points_index for `cap` rows per scan: 1 or 2"""
    return 1 if _device_cap(cap) < 1 << INDEX_DIGIT_BITS else 2


def max_segments_of(count):
    return max(1, -(-int(np.max(count)) // INDEX_SEGMENT))


# ---------------------------------------------------------------------------------- the rule in numpy
def host_point_index(keys, offset, count, cap):
    """The rule of the module docstring in numpy: keys (P,) integers flat over the scans, offset and
    count (S,) -> {start (S, cap + 1) int32, order (P,) int32}.  Rows of `order` that belong to no
    scan are -1."""
    cap = _cap(cap)
    keys = np.asarray(keys)
    if keys.ndim != 1 or keys.dtype.kind not in "iu":
        raise ValueError("host_point_index: keys must be a flat integer array, got %s %s" % (keys.dtype, keys.shape))
    offset, count = np.asarray(offset, np.int64), np.asarray(count, np.int64)
    if offset.ndim != 1 or offset.shape != count.shape or len(count) < 1:
        raise ValueError("host_point_index: offset %s and count %s must be (S,), S >= 1" % (offset.shape, count.shape))
    if (count < 0).any() or (offset < 0).any() or (offset + count > len(keys)).any():
        raise ValueError("host_point_index: a scan's rows leave the %d keys" % len(keys))
    start = np.zeros((len(count), cap + 1), np.int32)
    order = np.full(len(keys), -1, np.int32)
    for s, (o, n) in enumerate(zip(offset, count)):
        k = keys[o:o + n].astype(np.int64)
        b = np.where((k >= 0) & (k < cap), k, cap)
        order[o:o + n] = np.argsort(b, kind="stable")
        start[s, 1:] = np.cumsum(np.bincount(b, minlength=cap + 1)[:cap])
    return {"start": start, "order": order}


# ---------------------------------------------------------------------------------- the launch
def index_scratch_bytes(S, cap, max_segments, P):
    """scene_points_index_scratch_bytes"""
    from .. import _lib
    return int(_lib.lib.scene_points_index_scratch_bytes(S, cap, max_segments, P))


def index_record(key, offset, count, cap, max_segments, start, order, scratch):
    a = records.PointsIndexArgs()
    a.S, a.cap, a.max_segments, a.P = offset.shape[0], cap, max_segments, key.shape[0]
    a.key, a.offset, a.count = key.data_ptr(), offset.data_ptr(), count.data_ptr()
    a.start, a.order, a.scratch = start.data_ptr(), order.data_ptr(), scratch.data_ptr()
    a.scratch_bytes = scratch.numel() * scratch.element_size()
    return a


def point_index_gpu(key, offset, count, cap, start=None, order=None, scratch=None, max_segments=None):
    """Launch scene_points_index over device planes key (P,) int32, offset (S,) int64, count (S,) int32
    -> (start (S, cap + 1) int32, order (P,) int32, scratch: bytes).  The three outputs may be
    given; they may hold anything.  `max_segments`: ceil(largest count / INDEX_SEGMENT) where the caller
    knows the counts on the host (max_segments_of); by default the bound every scan meets,
    ceil(P / INDEX_SEGMENT), so that nothing is read back."""
    from .. import _lib
    cap = _device_cap(cap)
    if key.dtype != torch.int32 or key.dim() != 1 or not key.is_contiguous() or key.shape[0] < 1:
        raise ValueError("point_index_gpu: key must be a contiguous (P,) int32 tensor, P >= 1")
    if offset.dtype != torch.int64 or count.dtype != torch.int32 or offset.dim() != 1 or offset.shape != count.shape:
        raise ValueError("point_index_gpu: offset (S,) int64 and count (S,) int32")
    S, P, dev = offset.shape[0], key.shape[0], key.device
    if max_segments is None:
        max_segments = max(1, -(-P // INDEX_SEGMENT))
    if start is None:
        start = torch.empty((S, cap + 1), dtype=torch.int32, device=dev)
    if order is None:
        order = torch.empty(P, dtype=torch.int32, device=dev)
    if scratch is None:
        scratch = torch.empty(index_scratch_bytes(S, cap, max_segments, P), dtype=torch.uint8, device=dev)
    _lib.run("scene_points_index", index_record(key, offset, count, cap, max_segments, start, order, scratch), dev)
    return start, order, scratch


# ---------------------------------------------------------------------------------- the result
class PointIndex(object):
    """PointLabels.index()'s result.  `start` (S, cap + 1) and `order` (P,) int32 are device tensors
    (numpy arrays on the host path); `count`, `offset` are the store's host planes.  Indexing, by_name,
    points_of, lists and owned read the host copy, made once."""

    def __init__(self, names, count, offset, cap, start, order):
        self.names, self.count, self.offset, self.cap = list(names), count, offset, _cap(cap)
        self.start, self.order = start, order
        self._host, self._rows, self._words = None, None, None  # _words: start | order where they share a buffer

    def __len__(self):
        return len(self.names)

    def host(self):
        """{start, order}: numpy views of the one host copy."""
        if self._host is None:
            S, cut = len(self.names), len(self.names) * (self.cap + 1)
            if torch.is_tensor(self.start):
                w = self._words if self._words is not None else torch.cat([self.start.reshape(-1), self.order])
                w = w.cpu().numpy()
                self._host = {"start": w[:cut].reshape(S, self.cap + 1), "order": w[cut:]}
            else:
                self._host = {"start": self.start, "order": self.order}
        return self._host

    def _scan(self, i):
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        return i % len(self)

    def __getitem__(self, i):
        i = self._scan(i)
        h, o, n = self.host(), int(self.offset[i]), int(self.count[i])
        return {"start": h["start"][i], "order": h["order"][o:o + n]}

    def by_name(self, name):
        return self[self.names.index(name)]

    def points_of(self, i, row):
        """The indices, in scan i, of the points that packed row `row` owns, ascending: a slice."""
        row = int(row)
        if not 0 <= row < self.cap:
            raise IndexError("row %d of %d" % (row, self.cap))
        one = self[i]
        return one["order"][one["start"][row]:one["start"][row + 1]]

    def lists(self, i):
        """(rows, [indices of each]): the rows of scan i that own a point, ascending, and their lists."""
        one = self[i]
        rows = np.nonzero(np.diff(one["start"]))[0]
        return rows, [one["order"][one["start"][r]:one["start"][r + 1]] for r in rows]

    def owned(self, i):
        """The indices of scan i's owned points, grouped by row: order up to start[i, cap]."""
        one = self[i]
        return one["order"][:one["start"][self.cap]]

    def gather(self, cloud):
        """The store's rows (P, C) permuted so that every object's points are contiguous, scan by scan:
        cloud[offset + order], one index_select; on the device for a device index."""
        if self._rows is None:
            flat = np.repeat(np.asarray(self.offset, np.int64), np.asarray(self.count, np.int64))
            if torch.is_tensor(self.order):
                self._rows = torch.from_numpy(flat).to(self.order.device) + self.order
            else:
                self._rows = flat + self.order
        if len(cloud) != len(self._rows):
            raise ValueError("gather: %d rows, the index has %d" % (len(cloud), len(self._rows)))
        if torch.is_tensor(self._rows):
            return torch.index_select(cloud, 0, self._rows)
        return np.asarray(cloud)[self._rows]


def build_index(names, count, offset, cap, instance):
    """PointIndex of the label plane `instance` (P,) over the store's host planes `count`, `offset`: on
    the device where the labels are device tensors, else in numpy."""
    cap = _cap(cap)
    if not torch.is_tensor(instance):
        got = host_point_index(instance, offset, count, cap)
        return PointIndex(names, count, offset, cap, got["start"], got["order"])
    dev, S = instance.device, len(names)
    offset_dev = torch.from_numpy(np.ascontiguousarray(offset, np.int64)).to(dev)
    count_dev = torch.from_numpy(np.ascontiguousarray(count, np.int32)).to(dev)
    cut = S * (cap + 1)
    words = torch.empty(cut + instance.shape[0], dtype=torch.int32, device=dev)  # start | order
    start, order, _ = point_index_gpu(instance, offset_dev, count_dev, cap, start=words[:cut].view(S, cap + 1),
                                      order=words[cut:], max_segments=max_segments_of(count))
    index = PointIndex(names, count, offset, cap, start, order)
    index._words = words
    return index
