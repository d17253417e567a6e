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
    ]


ENTRY_POINTS = ["mlp_gemm_forward", "mlp_gemm_dgrad", "mlp_gemm_wgrad", "mlp_gemm_backward_small",
                "mlp_gemm_backward_fused", "mlp_pregather_backward"]


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_operand_validation_is_host_side(entry):
    load_pkg()
    K = importlib.import_module("pointnet2._mlp_ext")
    lib = K._lib
    name, dy_modes, x_modes, call = _calls()[ENTRY_POINTS.index(entry)]
    assert name == entry
    good_dy = _op(K, dy_modes[0]) if dy_modes else None
    good_x = _op(K, x_modes[0]) if x_modes else None
    bad = []
    for modes, slot in ((dy_modes, "dy"), (x_modes, "x")):
        if modes is None:
            continue
        for mode in (-1, 0, 1, 2, 3, 4, 5):
            if mode not in modes:
                bad.append((slot, _op(K, mode), "mode %d" % mode))
        if 2 in modes:
            bad.append((slot, _op(K, 2, drop=("coef",)), "mode 2 without coef"))
        if 3 in modes:
            bad.append((slot, _op(K, 3, ns=0), "mode 3 with ns = 0"))
        if 1 in modes:
            bad.append((slot, _op(K, 1, drop=("shift",)), "mode 1 without shift"))
        bad.append((slot, _op(K, modes[0], drop=("x",)), "no tensor"))
    assert bad
    for slot, op, what in bad:
        dy, x = (op, good_x) if slot == "dy" else (good_dy, op)
        assert call(lib, 8, dy, x) == INVALID, "%s: %s as %s" % (name, what, slot)
        assert call(lib, 0, dy, x) == 0, "%s: empty shape, %s as %s" % (name, what, slot)
    # a missing record is refused like a bad one
    if dy_modes:
        assert call(lib, 8, None, good_x) == INVALID
    if x_modes:
        assert call(lib, 8, good_dy, None) == INVALID


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
