"""CPU tests of the operand record of the shared-MLP GEMMs (include/mlp_hip.h, MlpOperand): the
ctypes mirror has the header's fields in the header's order, and every entry point that takes a
record checks it on the host -- a mode it does not take, or a mode whose fields are not all there,
is hipErrorInvalidValue before anything is launched (no device needed: the calls below return from
the check, their dummy addresses are never dereferenced)."""
import ctypes
import importlib
import os
import re

import pytest

from conftest import ROOT, load_pkg

INVALID = 1  # hipErrorInvalidValue
CTYPE = {"int": ctypes.c_int, "const float *": ctypes.c_void_p, "const int *": ctypes.c_void_p}


def _header_fields():
    """[(type, name)] of MlpOperand as include/mlp_hip.h declares it"""
    text = open(os.path.join(ROOT, "include", "mlp_hip.h")).read()
    body = text[text.index("typedef struct MlpOperand {"):text.index("} MlpOperand;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            m = re.fullmatch(r"(.*?[ *])([A-Za-z_][A-Za-z_0-9]*)", decl)
            fields.append((m.group(1).strip(), m.group(2)))
    return fields


def test_operand_struct_matches_header():
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    fields = _header_fields()
    assert [n for _, n in fields] == [n for n, _ in K.MlpOperand._fields_]
    assert [t for t, _ in fields] == ["int"] + ["const float *"] * 7 + ["const int *", "int", "int",
                                                                      "const float *"]
    size = align = 0
    for t, _ in fields:  # natural alignment: every field at a multiple of its size
        s = ctypes.sizeof(CTYPE[t])
        size = (size + s - 1) // s * s + s
        align = max(align, s)
    size = (size + align - 1) // align * align
    assert ctypes.sizeof(K.MlpOperand) == size
    for (t, n), (_, ct) in zip(fields, K.MlpOperand._fields_):
        assert ctypes.sizeof(ct) == ctypes.sizeof(CTYPE[t]), n


# dummy non-NULL device addresses: the checks return before any of them is read
A = 0x1000


def _op(K, mode, drop=(), **over):
    full = dict(x=A, dz=A, scale=A, shift=A, mean=A, invstd=A, coef=A, argmax=A, lin_w=A, ns=4, groups=16)
    full.update(over)
    for name in drop:
        full[name] = None
    return K.MlpOperand(mode=mode, **full)


# (entry point, modes of dy or None, modes of x or None, call(lib, b, dy, x)); r = 64 = groups * ns
# unless the call says otherwise (the pooled entry points: r = groups * 64, their _op(ns=64, groups=...))
def _calls():
    def ref(op):
        return ctypes.byref(op) if op is not None else None
    return [
        ("mlp_gemm_forward", None, (0, 1),
         lambda lib, b, dy, x: lib.mlp_gemm_forward(b, 64, 64, 64, A, None, ref(x), A, None, None)),
        ("mlp_gemm_dgrad", (0, 2, 3), None,
         lambda lib, b, dy, x: lib.mlp_gemm_dgrad(b, 64, 64, 64, A, ref(dy), A, None)),
        ("mlp_gemm_wgrad", (0, 2, 3), (0, 1),
         lambda lib, b, dy, x: lib.mlp_gemm_wgrad(b, 64, 64, 64, ref(dy), ref(x), A, A, None)),
        ("mlp_gemm_backward_small", (0, 2), (0, 1),
         lambda lib, b, dy, x: lib.mlp_gemm_backward_small(b, 64, 64, 64, A, None, ref(dy), ref(x), A, A,
                                                           A, None)),
        ("mlp_gemm_backward_fused", (2, 3), (0, 1, 4),
         lambda lib, b, dy, x: lib.mlp_gemm_backward_fused(b, 64, 64, 64, A, ref(dy), ref(x), A, A, A,
                                                           None, None)),
        ("mlp_pregather_backward", (2,), None,
         lambda lib, b, dy, x: lib.mlp_pregather_backward(b, 64, 128, 16, 4, ref(dy), A, A, None)),
        ("mlp_gemm_forward_stats_pool", None, (1,),
         lambda lib, b, dy, x: lib.mlp_gemm_forward_stats_pool(b, *POOL_SHAPE, A, ref(x), A, A, 64, A, A, None)),
        ("mlp_pool_gram_backward", (3,), (1,),
         lambda lib, b, dy, x: lib.mlp_pool_gram_backward(b, *GRAM_SHAPE, A, ref(dy), ref(x), A, A, A, A, A,
                                                          None)),
    ]


POOL_SHAPE = (128, 64, 4096)  # (m, k, r) at b = 8, ns = 64: 32768 columns, past the small-GEMM regime
GRAM_SHAPE = (128, 64, 256)   # (m, k, r) at b = 8, ns = 64, groups = 4: 64 chunks of 32 columns
# per entry point: what _op() must carry for a mode-3 record to fit the call's r
GEOMETRY = {"mlp_pool_gram_backward": dict(ns=64, groups=4)}
# an empty shape returns 0 whatever the record -- but mlp_gemm_forward_stats_pool's shape gate comes
# before everything else and refuses b = 0: nothing is launched either way
EMPTY_OK = {"mlp_gemm_forward_stats_pool": (0, INVALID)}
# mlp_pool_gram_backward's dy carries no tensor (the raw output was never stored): NULL x is valid
X_OPTIONAL = {("mlp_pool_gram_backward", "dy")}


ENTRY_POINTS = ["mlp_gemm_forward", "mlp_gemm_dgrad", "mlp_gemm_wgrad", "mlp_gemm_backward_small",
                "mlp_gemm_backward_fused", "mlp_pregather_backward", "mlp_gemm_forward_stats_pool",
                "mlp_pool_gram_backward"]


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_operand_validation_is_host_side(entry):
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    lib = K._lib
    name, dy_modes, x_modes, call = _calls()[ENTRY_POINTS.index(entry)]
    assert name == entry
    if entry == "mlp_gemm_forward_stats_pool":  # the shape gate must pass, or the record is never looked at
        assert lib.mlp_gemm_forward_stats_pool_supported(8, *POOL_SHAPE, 64) == 1
    if entry == "mlp_pool_gram_backward":
        assert lib.mlp_pool_gram_supported(8, *GRAM_SHAPE, 64) == 1
    geo = GEOMETRY.get(entry, {})

    def rec(mode, drop=(), **over):
        return _op(K, mode, drop, **dict(geo, **over))
    good_dy = rec(dy_modes[0]) if dy_modes else None
    good_x = rec(x_modes[0]) if x_modes else None
    bad = []
    for modes, slot in ((dy_modes, "dy"), (x_modes, "x")):
        if modes is None:
            continue
        for mode in (-1, 0, 1, 2, 3, 4, 5):
            if mode not in modes:
                bad.append((slot, rec(mode), "mode %d" % mode))
        if 2 in modes:
            bad.append((slot, rec(2, drop=("coef",)), "mode 2 without coef"))
        if 3 in modes:
            bad.append((slot, rec(3, ns=0), "mode 3 with ns = 0"))
        if 1 in modes:
            bad.append((slot, rec(1, drop=("shift",)), "mode 1 without shift"))
        if (entry, slot) not in X_OPTIONAL:
            bad.append((slot, rec(modes[0], drop=("x",)), "no tensor"))
    assert bad
    for slot, op, what in bad:
        dy, x = (op, good_x) if slot == "dy" else (good_dy, op)
        assert call(lib, 8, dy, x) == INVALID, "%s: %s as %s" % (name, what, slot)
        assert call(lib, 0, dy, x) in EMPTY_OK.get(entry, (0,)), \
            "%s: empty shape, %s as %s" % (name, what, slot)
    # a missing record is refused like a bad one
    if dy_modes:
        assert call(lib, 8, None, good_x) == INVALID
    if x_modes:
        assert call(lib, 8, good_dy, None) == INVALID


def test_pooled_gram_backward_takes_its_two_records_and_nothing_else():
    """mlp_pool_gram_backward: dy mode 3 only, x mode 1 only with mean / invstd, (m, k) one of the two
    covered layers.  Its mode-3 record carries no x (the raw output was never stored): with x = NULL the
    call gets as far as the next check -- here ymax = NULL, which refuses it before any launch, as it
    refuses the same call with x given; the record itself, alone among the entry points, passes
    (mlp_gemm_dgrad refuses it)."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    lib = K._lib
    assert lib.mlp_pool_gram_supported(8, *GRAM_SHAPE, 64) == 1
    dy, x = _op(K, 3, ns=64, groups=4), _op(K, 1)

    def call(dy, x, m=128, k=64, ymax=A):
        return lib.mlp_pool_gram_backward(8, m, k, 256, A, ctypes.byref(dy), ctypes.byref(x), ymax, A, A, A,
                                          A, None)
    for mode in (-1, 0, 1, 2, 4, 5):
        assert call(_op(K, mode, ns=64, groups=4), x) == INVALID, "dy mode %d" % mode
    for mode in (-1, 0, 2, 3, 4, 5):
        assert call(dy, _op(K, mode, ns=64, groups=4)) == INVALID, "x mode %d" % mode
    assert call(_op(K, 3, drop=("coef",), ns=64, groups=4), x) == INVALID
    assert call(_op(K, 3, ns=0, groups=4), x) == INVALID
    assert call(_op(K, 3, ns=64, groups=2), x) == INVALID  # groups * ns != r
    assert call(dy, _op(K, 1, drop=("mean",))) == INVALID
    assert call(dy, _op(K, 1, drop=("invstd",))) == INVALID
    assert call(dy, x, m=128, k=128) == INVALID
    no_x = _op(K, 3, drop=("x",), ns=64, groups=4)
    assert call(no_x, x, ymax=None) == INVALID
    assert call(dy, x, ymax=None) == INVALID
    assert lib.mlp_gemm_dgrad(8, 128, 64, 256, A, ctypes.byref(no_x), A, None) == INVALID
    # the other three of the family: one dispatch on (m, k)
    assert lib.mlp_pool_gram_supported(8, 128, 128, 256, 64) == 0
    assert lib.mlp_pool_gram_parts(8, 128, 128, 256) == 0
    assert lib.mlp_pool_gram_workspace_floats(8, 128, 128, 256, 64) == 0
    assert lib.mlp_pool_gram_parts(8, *GRAM_SHAPE) > 0 and lib.mlp_pool_gram_parts(8, 256, 128, 256) > 0
    assert lib.mlp_pool_gram_workspace_floats(8, *GRAM_SHAPE, 64) > 0
    assert lib.mlp_pool_gram_workspace_floats(8, 256, 128, 256, 16) > 0


def test_forward_with_a_virtual_first_layer_below():
    """mlp_gemm_forward, x in mode 4: only with pairs, only (64, 64), only with lin_w."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    lib = K._lib
    x = _op(K, 4)
    assert lib.mlp_gemm_forward_stats_parts(8, 64, 64, 4096, None) > 0
    assert lib.mlp_gemm_forward_stats_parts(8, 128, 64, 4096, None) > 0
    assert lib.mlp_gemm_forward(8, 64, 64, 4096, A, None, ctypes.byref(x), A, None, None) == INVALID
    assert lib.mlp_gemm_forward(8, 128, 64, 4096, A, None, ctypes.byref(x), A, A, None) == INVALID
    no_w = _op(K, 4, drop=("lin_w",))
    assert lib.mlp_gemm_forward(8, 64, 64, 4096, A, None, ctypes.byref(no_w), A, A, None) == INVALID
    assert lib.mlp_gemm_forward(8, 64, 64, 4096, A, None, ctypes.byref(_op(K, 4, lin_w=A + 4)), A, A,
                                None) == INVALID  # lin_w not 16-byte aligned
    assert lib.mlp_gemm_forward(0, 64, 64, 4096, A, None, ctypes.byref(no_w), A, A, None) == 0


def test_forward_takes_an_image_or_statistics_not_both():
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    x = _op(K, 1)
    both = lambda b: K._lib.mlp_gemm_forward(b, 64, 64, 64, A, A, ctypes.byref(x), A, A, None)
    assert both(8) == INVALID
    assert both(0) == 0



def test_binding_refuses_anything_but_a_record_where_an_operand_belongs():
    """The operand arguments are typed pointers in the ctypes binding: an integer or a raw address in
    their place -- the positional argument lists these entry points had before the record, a mode
    number where `dy` belongs -- raises before the call; the library never sees it as an address."""
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    lib = K._lib
    x = _op(K, 1)
    with pytest.raises(ctypes.ArgumentError):  # (b, m, k, r, w, pmode, y, dz, argmax, ns, scale, ...)
        lib.mlp_gemm_backward_fused(8, 128, 128, 64, A, 2, A, A, None, 0, A, A, A, A, A, 1, A, A, A, A, A, None,
                                    A, A, A, None, None)
    with pytest.raises(ctypes.ArgumentError):  # (b, m, k, r, w, x, mode, scale, shift, y, stream)
        lib.mlp_gemm_forward(8, 64, 64, 64, A, A, 1, A, A, A, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.mlp_gemm_dgrad(8, 64, 64, 64, A, A, A, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.mlp_gemm_wgrad(8, 64, 64, 64, 2, ctypes.byref(x), A, A, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.mlp_gemm_backward_small(8, 64, 64, 64, A, None, A, ctypes.byref(x), A, A, A, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.mlp_pregather_backward(8, 64, 128, 16, 4, A, A, A, A, A, A, A, A, A, None)
    with pytest.raises(ctypes.ArgumentError):  # (b, r, ns, w3, y2, sc2, ..., workspace, stream): 3 + 19
        lib.mlp_pool_gram_backward(8, 256, 64, *([A] * 18), None)
    with pytest.raises(ctypes.ArgumentError):  # (b, m, k, r, w, x, scale, shift, y, pairs, ns, gamma, ext, stream)
        lib.mlp_gemm_forward_stats_pool(8, 128, 64, 4096, A, A, A, A, A, A, 64, A, A, None)
