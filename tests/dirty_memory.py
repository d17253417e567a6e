"""Run a binding on dirty memory: inside `with poisoned(fill):` every tensor the Python bindings
allocate with torch.empty / torch.empty_like / Tensor.new_empty arrives filled with `fill` instead
of whatever the allocator happened to hand back (in the tests: a fresh zero page, or the block the
same test wrote a moment ago).  A kernel that leaves an element of its output unwritten, reads a
partial an idle workgroup never wrote, multiplies a padded row by zero or accumulates into its
output then shows: the result is not finite, or differs between two fills.

    with poisoned(float("nan")) as p:
        out = K.gemm_forward(w, x)
    assert p.count > 0            # p.count allocations, p.bytes bytes were filled

A plain module the tests import (not a conftest, no fixture).  Only the three Python names are
replaced; torch's internal C++ allocations (the outputs of torch's own operators) are untouched.

What is filled
  * float32 / float64 results, non-empty: with `fill`.  FILLS are the three values every case runs
    under: NaN, and two huge finite values of opposite sign -- fmaxf / fminf drop a NaN, so an
    extremum seeded from garbage would hide it, and the two make an unwritten element differ
    between runs.
  * integer, bool and byte results: NOT filled.  Many hold indices, counts or offsets (the FPS and
    cell-list workspaces, group_inverse, argmax, object_assignment, the head of the lhs_pseudo_stats
    workspace); garbage there read by a wrong kernel is an out-of-bounds access, not a wrong number.
  * byte / int16 buffers on the allow-list `byte_sites`: with 0xFF bytes (a NaN as bf16, float and
    double alike).  A site is named by its size function: a uint8 / int8 / int16 allocation is
    filled when the source of the calling function, up to the line of the call, names a listed
    function.  A buffer is listed only where the project's comments say it holds floating-point
    data or bf16 images and nothing else.

Every byte workspace of the bindings:
  mlp_chain_lin4_image_bytes           LISTED  [W2][W3T] bf16 images + float tables (w1 rows, sc1,
                                               sh1): csrc/mlp_frag.h kLin4ImgBytes, include/mlp_hip.h
                                               "fragment-ordered bf16 images"
  mlp_eval_stored_image_bytes          LISTED  "fragment-ordered bf16 images (exact three-term
                                               split)" of w1 and w2, nothing else
  mlp_weight_image_elems (int16 buf)   LISTED  "three planes, both dimensions padded to multiples
                                               of 64" of 2-byte bf16 elements
  mlp_bn_finalize_pairs_scratch_bytes  LISTED  sizeof(double) * 3 * slices * c: doubles only
  mlp_wgrad_first4_workspace_bytes     left    floats then doubles by csrc/mlp_first4.hip, but the
                                               header only calls it "the workspace": not stated
  pn2_* workspaces of _ext.py          left    FPS buckets, cell lists, group_inverse, sort keys:
  (ws, buf, gbuf: all uint8)                   counts, offsets and point indices
  lhs_pseudo_stats_workspace_bytes     left    "it starts with the (S,K) int32 first GT index of
                                               every IoU label" (include/lhs_hip.h)
"""
import contextlib
import linecache
import sys

import torch

NAN = float("nan")
FILLS = (NAN, 3.0e38, -3.0e38)
FILL_IDS = ("nan", "+3e38", "-3e38")

BYTE_SITES = (
    "mlp_chain_lin4_image_bytes",
    "mlp_eval_stored_image_bytes",
    "mlp_weight_image_elems",
    "mlp_bn_finalize_pairs_scratch_bytes",
)

_FLOAT = (torch.float32, torch.float64)
_BYTE = (torch.uint8, torch.int8, torch.int16)


class Poison(object):
    """What one `poisoned` block filled: `count` allocations, `bytes` bytes in all."""

    def __init__(self, fill, byte_sites):
        self.fill = fill
        self.byte_sites = tuple(byte_sites)
        self.count = 0
        self.bytes = 0
        self.byte_count = 0  # of `count`: the allow-listed byte / int16 buffers

    def _site_listed(self, frame):
        if not self.byte_sites or frame is None:
            return False
        code = frame.f_code
        lines = [linecache.getline(code.co_filename, n, frame.f_globals)
                 for n in range(code.co_firstlineno, frame.f_lineno + 1)]
        text = "".join(lines)
        return any(name in text for name in self.byte_sites)

    def touch(self, t, frame):
        if not isinstance(t, torch.Tensor) or t.numel() == 0:
            return t
        if t.dtype in _FLOAT:
            t.fill_(self.fill)
        elif t.dtype in _BYTE and self._site_listed(frame):
            t.view(torch.uint8).fill_(0xFF)
            self.byte_count += 1
        else:
            return t
        self.count += 1
        self.bytes += t.numel() * t.element_size()
        return t


@contextlib.contextmanager
def poisoned(fill, byte_sites=BYTE_SITES):
    """Replace torch.empty, torch.empty_like and torch.Tensor.new_empty by wrappers that call the
    real function with the same arguments and then fill the result (see the module docstring);
    the originals come back at exit, also when the block raises.  Yields the Poison record."""
    record = Poison(fill, byte_sites)
    real_empty, real_empty_like, real_new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def empty(*args, **kwargs):
        return record.touch(real_empty(*args, **kwargs), sys._getframe(1))

    def empty_like(*args, **kwargs):
        return record.touch(real_empty_like(*args, **kwargs), sys._getframe(1))

    def new_empty(self, *args, **kwargs):
        return record.touch(real_new_empty(self, *args, **kwargs), sys._getframe(1))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield record
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = real_empty, real_empty_like, real_new_empty
