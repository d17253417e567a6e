"""tests/dirty_memory.py on the CPU: what `poisoned` fills, leaves alone, counts and restores -- and
the guard that keeps tests/test_dirty_memory_gpu.py from silently testing nothing: every
uninitialised allocation of the binding modules is spelt in one of the three ways the helper
replaces."""
import importlib
import inspect
import io
import math
import re
import tokenize

import pytest
import torch

from conftest import load_pkg
from dirty_memory import BYTE_SITES, FILLS, poisoned

BINDING_MODULES = [
    "pointnet2._mlp_ext",
    "pointnet2._ext",
    "pointnet2.pytorch_utils",
    "pointnet2.pointnet2_utils",
    "pcdet.ops.iou3d_nms.iou3d_nms_cuda",
    "pcdet.ops.iou3d_nms.iou3d_nms_utils",
    "3dioumatch_amd.votenet.fused_loss",
    "3dioumatch_amd.votenet.pseudo_nms",
    "3dioumatch_amd.votenet.heads",
    "3dioumatch_amd.votenet.detector",
    "3dioumatch_amd.votenet.iou_opt",
    "3dioumatch_amd.votenet.eval_det",
    "3dioumatch_amd.votenet.eval_helper",
    "3dioumatch_amd.votenet.fused_head",
]


def _same(t, fill):
    if math.isnan(fill):
        return bool(torch.isnan(t).all())
    return bool((t == fill).all())


@pytest.mark.parametrize("fill", FILLS)
def test_float_results_of_all_three_spellings_are_filled(fill):
    ref = torch.zeros(3, 5)
    with poisoned(fill) as p:
        a = torch.empty((4, 7), dtype=torch.float32)
        b = torch.empty(6, dtype=torch.float64)
        c = torch.empty_like(ref)
        d = ref.new_empty((2, 3))
        e = torch.empty_like(ref, dtype=torch.float64)
    for t in (a, b, c, d, e):
        assert _same(t, fill)
    assert (a.shape, a.dtype) == ((4, 7), torch.float32) and (b.shape, b.dtype) == ((6,), torch.float64)
    assert (c.shape, d.shape, e.dtype) == (ref.shape, (2, 3), torch.float64)
    assert p.count == 5 and p.byte_count == 0
    assert p.bytes == 4 * 28 + 8 * 6 + 4 * 15 + 4 * 6 + 8 * 15


def test_integer_bool_byte_and_empty_results_are_left_alone():
    ref = torch.zeros(3, dtype=torch.int64)
    marks = {}
    real_fill = torch.Tensor.fill_

    def spy(self, *args):
        marks[self.dtype] = True
        return real_fill(self, *args)

    torch.Tensor.fill_ = spy
    try:
        with poisoned(float("nan")) as p:
            torch.empty(5, dtype=torch.int32)
            torch.empty(5, dtype=torch.int64)
            torch.empty(5, dtype=torch.bool)
            torch.empty(5, dtype=torch.uint8)
            torch.empty(5, dtype=torch.int16)
            torch.empty_like(ref)
            ref.new_empty((4,))
            torch.empty(0, dtype=torch.float32)
            torch.empty(5, dtype=torch.bfloat16)  # (only float32 / float64 are data here)
    finally:
        torch.Tensor.fill_ = real_fill
    assert marks == {} and p.count == 0 and p.bytes == 0


def _alloc_listed(n):
    size = mlp_chain_lin4_image_bytes(n)
    return torch.empty(size, dtype=torch.uint8), torch.empty(size, dtype=torch.int16), \
        torch.empty(size, dtype=torch.int32)


def mlp_chain_lin4_image_bytes(n):  # (a stand-in with a listed size function's name)
    return n


def _alloc_unlisted(n):
    return torch.empty(n, dtype=torch.uint8)


def test_byte_buffers_are_filled_only_at_listed_sites():
    assert "mlp_chain_lin4_image_bytes" in BYTE_SITES
    with poisoned(float("nan")) as p:
        u8, i16, i32 = _alloc_listed(8)
        i32.zero_()
        other = _alloc_unlisted(8).zero_()
    assert bool((u8 == 0xFF).all()) and bool((i16 == -1).all())
    assert bool((i32 == 0).all()) and bool((other == 0).all())
    assert p.count == 2 and p.byte_count == 2 and p.bytes == 8 + 16
    with poisoned(float("nan"), byte_sites=()) as p:
        _alloc_listed(8)
    assert p.count == 0


def test_originals_come_back_after_exit_and_after_an_exception():
    originals = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with poisoned(1.0):
        assert torch.empty is not originals[0] and torch.empty_like is not originals[1]
        assert torch.Tensor.new_empty is not originals[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == originals
    with pytest.raises(KeyError):
        with poisoned(1.0):
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == originals
    with poisoned(2.0) as outer:  # nested blocks unwind in order
        with poisoned(3.0) as inner:
            t = torch.empty(2)
        u = torch.empty(2)
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == originals
    assert inner.count == 1 and outer.count == 2 and float(u[0]) == 2.0 and float(t[0]) == 3.0


def test_arguments_pass_through_unchanged():
    with poisoned(5.0):
        t = torch.empty(2, 3, dtype=torch.float64, requires_grad=False, pin_memory=False)
        out = torch.empty(6)
        u = torch.empty((2, 3), out=out.view(2, 3))
        v = torch.empty_like(t, memory_format=torch.contiguous_format)
    assert t.shape == (2, 3) and t.dtype == torch.float64 and float(t[1, 2]) == 5.0
    assert u.data_ptr() == out.data_ptr() and v.shape == t.shape


# ---- the allocation-spelling guard -----------------------------------------------------------
ALLOWED = {"torch.empty", "torch.empty_like", "new_empty"}
_CALL = re.compile(r"\btorch\.(?:cuda\.)?(\w+)\s*\(|\.(new(?:_\w+)?)\s*\(")
_LEGACY = re.compile(r"^(?:\w*Tensor|\w+Storage)$")
_ALIAS = re.compile(r"\btorch\.(?:Tensor\.)?(?:new_)?empty\w*\b(?!\s*\()")
_IMPORT = re.compile(r"\bfrom\s+torch(?:\.\w+)*\s+import\b(.*)")
_RENAMED = re.compile(r"^\s*import\s+torch\s+as\b|\bimport\b.*,\s*torch\s+as\b")


def _code_only(source):
    """`source` with every comment and string literal blanked out (same line numbers)"""
    lines = source.splitlines(True)
    for tok in tokenize.generate_tokens(io.StringIO(source).readline):
        if tok.type not in (tokenize.COMMENT, tokenize.STRING):
            continue
        (r0, c0), (r1, c1) = tok.start, tok.end
        for r in range(r0, r1 + 1):
            line = lines[r - 1]
            body = line.rstrip("\n")
            lo = c0 if r == r0 else 0
            hi = c1 if r == r1 else len(body)
            lines[r - 1] = body[:lo] + " " * (hi - lo) + body[hi:] + line[len(body):]
    return lines


def uninitialised_sites(source, filename):
    """-> (the spellings in use, the offending 'file:line: text' entries)"""
    used, bad = set(), []
    for number, line in enumerate(_code_only(source), 1):
        where = "%s:%d: %s" % (filename, number, line.strip())
        for m in _CALL.finditer(line):
            name = m.group(1)
            if name is not None:
                if "empty" in name:
                    used.add("torch." + name)
                    if "torch." + name not in ALLOWED:
                        bad.append(where)
                elif _LEGACY.match(name):
                    bad.append(where)
            else:
                name = m.group(2)
                if name == "new" or "empty" in name:
                    used.add(name)
                    if name not in ALLOWED:
                        bad.append(where)
        if _ALIAS.search(line):  # a reference kept at import time escapes the replacement
            bad.append(where)
        if _RENAMED.search(line):  # torch under another name: its calls would not match `torch.`
            bad.append(where)
        m = _IMPORT.search(line)
        if m and re.search(r"empty|Tensor\b|\*", m.group(1)):
            bad.append(where)
    return used, bad


@pytest.mark.parametrize("line", [
    "t = torch.empty_strided((2, 3), (3, 1))",
    "t = torch.Tensor(4)",
    "t = torch.FloatTensor(4, 5)",
    "t = torch.cuda.FloatTensor(4)",
    "t = x.new(3)",
    "t = x.new_empty_strided((2,), (1,))",
    "from torch import empty",
    "from torch import zeros, empty_like as el",
    "alloc = torch.empty",
    "import torch as th",
    "import os, torch as th",
    "t = torch._empty_affine_quantized((2,))",
])
def test_guard_rejects_other_spellings(line):
    source = "import numpy\n\n%s\n" % line
    _, bad = uninitialised_sites(source, "some/module.py")
    assert len(bad) == 1 and bad[0].startswith("some/module.py:3: "), bad


def test_guard_accepts_the_three_spellings_and_initialised_allocations():
    source = ('import torch\n"""torch.Tensor(3) in a docstring"""\n'
              "a = torch.empty((2,), dtype=torch.float32)  # not torch.empty_strided(\n"
              "b = torch.empty_like(a)\nc = a.new_empty((3,))\nd = torch.zeros(3)\n"
              "e = a.new_zeros(3)\nf = torch.zeros_like(a)\ng = isinstance(a, torch.Tensor)\n"
              "h = a.new_full((2,), 1.0)\ni = torch.full((2,), 0.0)\nj = a.new_tensor([1.0])\n")
    used, bad = uninitialised_sites(source, "m.py")
    assert bad == [] and used == ALLOWED


@pytest.mark.parametrize("name", BINDING_MODULES)
def test_bindings_allocate_only_through_the_replaced_names(name):
    load_pkg()
    module = importlib.import_module(name)
    source = inspect.getsource(module)
    used, bad = uninitialised_sites(source, inspect.getsourcefile(module))
    assert not bad, "allocations `poisoned` does not see:\n" + "\n".join(bad)
    assert used <= ALLOWED
