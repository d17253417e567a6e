"""CPU tests of the argument records of the C ABI (the `typedef struct X { ... } X;` of include/*.h, host
structs of device pointers): 3dioumatch_amd/records.py declares each of them once as a ctypes.Structure
with the header's name, fields, order, offsets and size, and _lib.py binds every `const <Record> *`
argument as a pointer to that class, so a record of another kind in its place is a ctypes.ArgumentError
before the call.  The records are discovered from the headers, not listed here; no device call."""
import ctypes
import glob
import importlib
import os
import re

import pytest

from conftest import ROOT, load_pkg

HEADERS = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
RECORDS_TODAY = 27  # the parser must find at least these: a parser that finds nothing checks nothing

# natural alignment: a scalar lies at a multiple of its size
SCALAR = {"int": 4, "unsigned": 4, "unsigned int": 4, "float": 4, "long long": 8, "unsigned long long": 8,
          "size_t": 8, "double": 8}
# ... and is mirrored by the ctypes class of its own kind: a float held as a c_int has the right offset too
CTYPE = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "float": ctypes.c_float,
         "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong, "size_t": ctypes.c_size_t,
         "double": ctypes.c_double}
POINTER = 8
TYPE_WORDS = {"const", "unsigned", "signed", "int", "long", "short", "char", "float", "double", "void", "size_t"}


def _text(path):
    text = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _defines():
    """{name: int} of the `#define NAME <integer expression>` of every header"""
    raw = {}
    for path in HEADERS:
        for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*)$", _text(path), re.M):
            raw[name] = value.strip()
    out = {}

    def value(name, seen=()):
        if name not in out:
            assert name in raw and name not in seen, "array bound %s is no #define of the headers" % name
            expr = re.sub(r"[A-Za-z_]\w*", lambda m: str(value(m.group(0), seen + (name,))), raw[name])
            assert re.fullmatch(r"[\d\s()<>+*/x-]+", expr), "%s = %s" % (name, raw[name])
            out[name] = int(eval(expr, {"__builtins__": {}}))
        return out[name]
    return value


def _parse_records():
    """{record: [(type, name, bounds)]} in the headers' order; type is the declared one without `const`,
    with a trailing '*' for a pointer; bounds is a tuple of ints (empty: no array)"""
    bound = _defines()
    found = []
    for path in HEADERS:
        for tag, body, name in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", _text(path), re.S):
            assert tag == name, "%s: typedef struct %s ... %s" % (os.path.basename(path), tag, name)
            found.append((name, body))
    names = {name for name, _ in found}
    assert len(names) == len(found), "a record is declared twice"
    records = {}
    for name, body in found:
        fields = []
        for decl in body.split(";"):
            words = decl.split()
            if not words:
                continue
            n = 0
            while n < len(words) and (words[n] in TYPE_WORDS or words[n] in names):
                n += 1
            base = " ".join(w for w in words[:n] if w != "const")
            assert base, "%s: no type in %r" % (name, decl)
            for declarator in "".join(words[n:]).split(","):
                m = re.fullmatch(r"((?:\*(?:const)?)*)(\w+)((?:\[\w+\])*)", declarator)
                assert m, "%s: cannot read the declarator %r" % (name, declarator)
                dims = tuple(int(d) if d.isdigit() else bound(d) for d in re.findall(r"\[(\w+)\]", m.group(3)))
                fields.append((base + (" *" if m.group(1) else ""), m.group(2), dims))
        assert fields, name
        records[name] = fields
    return records


RECORDS = _parse_records()


def _layout(record, memo={}):
    """(size, alignment, [(name, offset, size)]) of a record by natural alignment, from the header alone"""
    if record not in memo:
        at, align, rows = 0, 1, []
        for kind, name, dims in RECORDS[record]:
            if kind.endswith("*"):
                size = a = POINTER
            elif kind in RECORDS:
                size, a, _ = _layout(kind)
            else:
                assert kind in SCALAR, "%s.%s: type %r" % (record, name, kind)
                size = a = SCALAR[kind]
            for d in dims:
                size *= d
            at = (at + a - 1) // a * a
            rows.append((name, at, size))
            at += size
            align = max(align, a)
        memo[record] = ((at + align - 1) // align * align, align, rows)
    return memo[record]


def _records_module():
    load_pkg()
    return importlib.import_module("3dioumatch_amd.records")


def _declared_functions():
    """{function: [argument text]} of every function the headers declare"""
    out = {}
    for path in HEADERS:
        for name, args in re.findall(r"^[ \t]*(?:const char \*|long long|size_t|int)\s*\*?\s*(\w+)\s*\(([^)]*)\)\s*;",
                                     _text(path), re.M):
            out[name] = [" ".join(a.split()) for a in args.split(",")]
    return out


def test_the_parser_finds_the_records():
    assert len(HEADERS) >= 14
    assert len(RECORDS) >= RECORDS_TODAY
    for must in ("MlpOperand", "VnLossTensor", "VnLossArgs", "ScanVoxelArgs", "ScanSeamArgs", "SceneBatchArgs"):
        assert must in RECORDS
    # the forms the parser must read: comma-separated declarators, per-declarator stars, #defined bounds
    semi = {n: (t, d) for t, n, d in RECORDS["ScanSemiArgs"]}
    assert semi["seed"] == semi["counter"] == ("unsigned", ())
    assert semi["flip_x_axis"] == semi["flip_y_axis"] == ("long long *", ())
    assert semi["scene"][0] == "int" and len(semi["scene"][1]) == 1 and semi["scene"][1][0] > 1
    assert dict((n, (t, d)) for t, n, d in RECORDS["ScanVoxelArgs"])["voxel"] == ("double", (3,))
    assert dict((n, t) for t, n, _ in RECORDS["ScanVoxelCountArgs"])["mark"] == "ScanVoxelArgs"


def test_records_module_declares_exactly_the_headers_records():
    R = _records_module()
    have = {n for n, c in vars(R).items() if isinstance(c, type) and issubclass(c, ctypes.Structure)
            and c is not ctypes.Structure}
    assert have == set(RECORDS)
    for name in have:
        assert getattr(R, name).__name__ == name


def test_records_module_needs_ctypes_only():
    """records.py is importable where the host restatements are: it imports neither torch nor the library"""
    text = open(os.path.join(ROOT, "3dioumatch_amd", "records.py")).read()
    assert re.findall(r"^\s*(?:import|from)\s+(\S+)", text, re.M) == ["ctypes"]


@pytest.mark.parametrize("record", sorted(RECORDS))
def test_record_layout_matches_header(record):
    cls = getattr(_records_module(), record)
    size, _, rows = _layout(record)
    assert [n for n, _ in cls._fields_] == [n for _, n, _ in RECORDS[record]]
    for (name, offset, fsize), (kind, _, dims) in zip(rows, RECORDS[record]):
        field = getattr(cls, name)
        assert (field.offset, field.size) == (offset, fsize), "%s.%s" % (record, name)
        ctype = dict(cls._fields_)[name]
        for d in dims:  # an array field is an array, of the header's bounds
            assert issubclass(ctype, ctypes.Array) and ctype._length_ == d, "%s.%s" % (record, name)
            ctype = ctype._type_
        if kind.endswith("*"):
            assert ctype is ctypes.c_void_p, "%s.%s: a pointer is a c_void_p" % (record, name)
        elif kind in RECORDS:
            assert ctype is getattr(_records_module(), kind), "%s.%s: a nested record is nested" % (record, name)
        else:
            assert ctype is CTYPE[kind], "%s.%s: %s is a %s" % (record, name, kind, CTYPE[kind].__name__)
    assert ctypes.sizeof(cls) == size


def test_seam_record_extends_the_merge_record():
    R = _records_module()
    n = len(R.ScanMergeArgs._fields_)
    assert R.ScanSeamArgs._fields_[:n] == R.ScanMergeArgs._fields_ and len(R.ScanSeamArgs._fields_) > n


def test_the_operand_record_is_one_class():
    R = _records_module()
    L = importlib.import_module("3dioumatch_amd._lib")
    K = importlib.import_module("pointnet2._mlp_ext")
    assert L.MlpOperand is R.MlpOperand and K.MlpOperand is R.MlpOperand


def test_every_record_argument_is_bound_as_a_typed_pointer():
    R = _records_module()
    L = importlib.import_module("3dioumatch_amd._lib")
    bound = dict(L._SIGNATURES, **L._LOADER_SIGNATURES)
    functions = _declared_functions()
    assert set(functions) == set(bound)
    takers = 0
    for name, args in functions.items():
        argtypes = bound[name]
        if args == ["void"]:
            args = []
        assert len(argtypes) == len(args), name
        for i, (arg, ctype) in enumerate(zip(args, argtypes)):
            m = re.match(r"const (\w+) \*", arg)
            if m and m.group(1) in RECORDS:
                assert ctype is ctypes.POINTER(getattr(R, m.group(1))), "%s, argument %d: %s" % (name, i, arg)
                takers += 1
            else:
                assert not (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer)), \
                    "%s, argument %d is bound as a record, declared %s" % (name, i, arg)
        assert getattr(L.lib, name).argtypes == argtypes, name
    assert takers >= 30 + 9


def test_a_record_of_another_kind_is_refused_before_the_call():
    R = _records_module()
    L = importlib.import_module("3dioumatch_amd._lib")
    wrong = ctypes.byref(R.ScanTileCountArgs())
    for entry in ("scene_scan_voxel_count", "iou3d_eval_mark", "lhs_pseudo_select", "votenet_loss_forward_backward"):
        with pytest.raises(ctypes.ArgumentError):
            getattr(L.lib, entry)(wrong, None)
    with pytest.raises(ctypes.ArgumentError):
        L.lib.votenet_loss_scratch_floats(wrong)
    with pytest.raises(ctypes.ArgumentError):
        L.lib.votenet_eval_loss(ctypes.byref(R.VnLossTensor()), None, None, None)
    with pytest.raises(ctypes.ArgumentError):  # an address where a record belongs
        L.lib.scene_scan_tile_count(0x1000, None)
    # NULL still reaches the entry point, which refuses it itself (hipErrorInvalidValue)
    assert L.lib.scene_scan_tile_count(None, None) == 1
