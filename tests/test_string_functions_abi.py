"""The C ABI of the String functions without a GPU: the six entry points are declared, bound and exported, their contract is in the
header, every argument check that needs no device answers its code with a message in front of the device and writes nothing to the
outputs, the Python layer rejects wrong types before it touches the library, and the shim's members compile
(tests/string_functions_shim_driver.cpp, syntax only here)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOLS = {"chgpu_string_length": 5, "chgpu_string_map_case": 6, "chgpu_string_cmp_columns": 7, "chgpu_string_substring": 8, "chgpu_string_concat": 5,
           "chgpu_string_position_const": 6}
UNTOUCHED = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def K():
    from clickhouse_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


class FakeCol(C.Structure):
    """the head of a column as the library reads it in front of the device: {context, type, rows, data}"""
    _fields_ = [("ctx", C.c_void_p), ("type", C.c_int), ("rows", C.c_uint64), ("data", C.c_void_p), ("rest", C.c_uint64 * 8)]


def _col(tag, rows):
    return FakeCol(None, tag, rows, None)


def _p(col):
    return None if col is None else C.addressof(col)


class Outs:
    """output slots holding a pattern; .untouched() says no call wrote them"""

    def __init__(self, n):
        self.slots = [C.c_void_p(UNTOUCHED) for _ in range(n)]

    def refs(self):
        return [C.byref(s) for s in self.slots]

    def untouched(self):
        return all(s.value == UNTOUCHED for s in self.slots)


def _expect(K, rc, outs, code, word):
    assert rc == code, (rc, code)
    with pytest.raises(K.ChgpuError) as e:
        K.check(rc)
    assert e.value.code == code and word in str(e.value), str(e.value)
    assert outs.untouched()


@pytest.fixture()
def env(K):
    """a context that is looked at and never used by the checks in front of the device, and a ColumnString of 4 rows"""
    buf = C.create_string_buffer(1 << 16)
    env = dict(L=K.lib(), ctx=C.c_void_p(C.addressof(buf)), offs=_col(K.U64, 4), chars=_col(K.U8, 9), keep=buf)
    return env


def test_entry_points_are_declared_bound_and_exported(K):
    declared = K.declared_symbols()
    raw = C.CDLL(K.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert name in declared and name in K.SIGNATURES, name
        assert getattr(K.lib(), name) and getattr(raw, name)
        assert len(K.SIGNATURES[name][1]) == n_args, name
    assert C.sizeof(K.StringArg) == 32


def test_constants_and_contract_words_are_in_the_header(K):
    header = open(K.HEADER_PATH).read()
    for name in ("LENGTH", "LENGTH_UTF8", "EMPTY", "NOT_EMPTY", "LOWER", "UPPER"):
        assert f"CHGPU_STR_{name} = {getattr(K, 'STR_' + name)}" in header, name
    flat = " ".join(header.split())
    for words in ("(b & 0xC0) != 0x80", "bit 0x20 flipped", "substring('abc', -5, 3) = 'a'", "substring('abc', -5) = 'abc'", "substring('abc', 4) = ''",
                  "All arithmetic saturates", "offset == 0 answers CHGPU_ERR_NOT_IMPLEMENTED", "2 <= n_args <= 8", "The empty needle gives 1",
                  "is made before the first device call", "typedef struct chgpu_string_arg"):
        assert words in flat, words
    makefile = open(os.path.join(REPO, "clickhouse_amd", "csrc", "Makefile")).read()
    assert "string_func_kernels.hip" in makefile
    source = open(os.path.join(REPO, "clickhouse_amd", "csrc", "string_func_kernels.hip")).read()
    assert '#include "string_column.h"' in source
    for shared in ("str_column_begin", "str_call", "str_carve", "StrCols", "str_layout_values", "str_value", "str_load8", "str_copy_value"):
        assert shared in source, shared


def test_length_checks(K, env):
    L, ctx, offs, chars = env["L"], env["ctx"], env["offs"], env["chars"]
    bad = K.ERR_BAD_ARGUMENTS

    def f(ctx=ctx, o=offs, c=chars, kind=K.STR_LENGTH, out=True):
        outs = Outs(1)
        return L.chgpu_string_length(ctx, _p(o), _p(c), kind, outs.refs()[0] if out else None), outs

    for kw in (dict(ctx=None), dict(o=None), dict(c=None), dict(out=False)):
        _expect(K, *f(**kw), bad, "NULL")
    _expect(K, *f(o=_col(K.U32, 4)), bad, "UInt64 offsets")
    _expect(K, *f(c=_col(K.I8, 9)), bad, "UInt8 chars")
    for kind in (-1, 4, 99):
        _expect(K, *f(kind=kind), bad, "kind")


def test_map_case_checks(K, env):
    L, ctx, offs, chars = env["L"], env["ctx"], env["offs"], env["chars"]
    bad = K.ERR_BAD_ARGUMENTS

    def f(ctx=ctx, o=offs, c=chars, kind=K.STR_LOWER, oo=True, oc=True):
        outs = Outs(2)
        r = outs.refs()
        return L.chgpu_string_map_case(ctx, _p(o), _p(c), kind, r[0] if oo else None, r[1] if oc else None), outs

    for kw in (dict(ctx=None), dict(o=None), dict(c=None), dict(oo=False), dict(oc=False)):
        _expect(K, *f(**kw), bad, "NULL")
    _expect(K, *f(o=_col(K.I64, 4)), bad, "UInt64 offsets")
    for kind in (-1, 2):
        _expect(K, *f(kind=kind), bad, "kind")


def test_cmp_columns_checks(K, env):
    L, ctx, offs, chars = env["L"], env["ctx"], env["offs"], env["chars"]
    bad = K.ERR_BAD_ARGUMENTS

    def f(ctx=ctx, ao=offs, ac=chars, bo=offs, bc=chars, op=K.EQ, out=True):
        outs = Outs(1)
        return L.chgpu_string_cmp_columns(ctx, _p(ao), _p(ac), _p(bo), _p(bc), op, outs.refs()[0] if out else None), outs

    for kw in (dict(ctx=None), dict(ao=None), dict(ac=None), dict(bo=None), dict(bc=None), dict(out=False)):
        _expect(K, *f(**kw), bad, "NULL")
    _expect(K, *f(ac=_col(K.U16, 9)), bad, "UInt8 chars")
    _expect(K, *f(bo=_col(K.U32, 4)), bad, "UInt64 offsets")
    _expect(K, *f(bc=_col(K.U64, 9)), bad, "UInt8 chars")
    for op in (-1, 6):
        _expect(K, *f(op=op), bad, "comparison")
    for rows in (3, 5, 0):
        _expect(K, *f(bo=_col(K.U64, rows)), K.ERR_SIZES_MISMATCH, "rows")


def test_substring_checks(K, env):
    L, ctx, offs, chars = env["L"], env["ctx"], env["offs"], env["chars"]
    bad = K.ERR_BAD_ARGUMENTS

    def f(ctx=ctx, o=offs, c=chars, offset=1, has=0, length=0, oo=True, oc=True):
        outs = Outs(2)
        r = outs.refs()
        return L.chgpu_string_substring(ctx, _p(o), _p(c), offset, has, length, r[0] if oo else None, r[1] if oc else None), outs

    for kw in (dict(ctx=None), dict(o=None), dict(c=None), dict(oo=False), dict(oc=False)):
        _expect(K, *f(**kw), bad, "NULL")
    _expect(K, *f(c=_col(K.U32, 9)), bad, "UInt8 chars")
    for has, length in ((0, 0), (1, 0), (1, 5), (1, 2**64 - 1)):
        _expect(K, *f(offset=0, has=has, length=length), K.ERR_NOT_IMPLEMENTED, "offset 0")


def _args(K, *parts):
    """chgpu_string_arg[]: a (offsets, chars) pair of FakeCols is a column, bytes are a constant"""
    arr = (K.StringArg * max(len(parts), 1))()
    for slot, p in zip(arr, parts):
        if isinstance(p, bytes):
            slot.value, slot.value_bytes = p, len(p)
        else:
            slot.offsets, slot.chars = _p(p[0]), _p(p[1])
    return arr


def test_concat_checks(K, env):
    L, ctx, offs, chars = env["L"], env["ctx"], env["offs"], env["chars"]
    bad = K.ERR_BAD_ARGUMENTS
    col = (offs, chars)

    def f(*parts, ctx=ctx, n=None, args=True, oo=True, oc=True):
        outs = Outs(2)
        r = outs.refs()
        arr = _args(K, *parts)
        return L.chgpu_string_concat(ctx, arr if args else None, len(parts) if n is None else n, r[0] if oo else None, r[1] if oc else None), outs

    for kw in (dict(ctx=None), dict(args=False), dict(oo=False), dict(oc=False)):
        _expect(K, *f(col, col, **kw), bad, "NULL")
    _expect(K, *f(n=0), bad, "arguments")
    _expect(K, *f(col), bad, "arguments")
    _expect(K, *f(*([col] * 9)), bad, "arguments")
    _expect(K, *f(b"a", b"b"), bad, "at least one argument is a column")
    _expect(K, *f(b"", b"", b""), bad, "at least one argument is a column")
    _expect(K, *f(col, (offs, None)), bad, "NULL")
    _expect(K, *f((offs, None), col), bad, "NULL")
    _expect(K, *f(col, (_col(K.U32, 4), chars)), bad, "UInt64 offsets")
    _expect(K, *f((offs, _col(K.I8, 9)), b"x"), bad, "UInt8 chars")
    for rows in (3, 5, 0):
        _expect(K, *f(col, b"/", (_col(K.U64, rows), chars)), K.ERR_SIZES_MISMATCH, "rows")
    big = K.STR_CONST_MAX
    _expect(K, *f(col, b"x" * (big + 1)), K.ERR_NOT_IMPLEMENTED, "constant bytes")
    _expect(K, *f(b"x" * big, col, b"y"), K.ERR_NOT_IMPLEMENTED, "constant bytes")
    _expect(K, *f(*([b"x" * (big // 4)] * 4), col, b"\0"), K.ERR_NOT_IMPLEMENTED, "constant bytes")
    # a constant of some bytes and no pointer
    arr = _args(K, col, b"")
    arr[1].value, arr[1].value_bytes = None, 3
    outs = Outs(2)
    _expect(K, L.chgpu_string_concat(ctx, arr, 2, *outs.refs()), outs, bad, "NULL")


def test_position_checks(K, env):
    L, ctx, offs, chars = env["L"], env["ctx"], env["offs"], env["chars"]
    bad = K.ERR_BAD_ARGUMENTS

    def f(ctx=ctx, o=offs, c=chars, needle=b"ab", n=None, out=True):
        outs = Outs(1)
        return L.chgpu_string_position_const(ctx, _p(o), _p(c), needle, len(needle or b"") if n is None else n, outs.refs()[0] if out else None), outs

    for kw in (dict(ctx=None), dict(o=None), dict(c=None), dict(out=False), dict(needle=None, n=2)):
        _expect(K, *f(**kw), bad, "NULL")
    _expect(K, *f(o=_col(K.F64, 4)), bad, "UInt64 offsets")
    _expect(K, *f(needle=b"x" * (K.STR_CONST_MAX + 1)), K.ERR_NOT_IMPLEMENTED, "needle")


def test_python_rejects_wrong_types_before_the_library(K, monkeypatch):
    import numpy as np
    from clickhouse_amd.lowcardinality import ColumnString

    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(K, "lib", touched)
    s = ColumnString.__new__(ColumnString)
    for needle in (5, 1.5, None, ["a"], np.zeros(2, dtype=np.uint8), s):
        with pytest.raises(TypeError):
            s.position(needle)
    for other in (b"abc", "abc", None, 3):
        with pytest.raises(TypeError):
            s.compare_column(K.EQ, other)
    with pytest.raises(TypeError):
        s.compare_column("==", s)
    for offset, length in ((1.0, None), ("1", None), (None, None), (1, 2.0), (1, "2"), (True, None), (b"1", 1)):
        with pytest.raises(TypeError):
            s.substring(offset, length)
    for offset, length in ((2**63, None), (-2**63 - 1, None), (1, -1), (1, 2**64)):
        with pytest.raises(ValueError):
            s.substring(offset, length)
    for args in ((s, 5), (s, None), (1.5, s), (s, [b"a"]), (s, b"a", object())):
        with pytest.raises(TypeError):
            ColumnString.concat(*args)
    for args in ((), (b"a", "b"), (b"only",)):
        with pytest.raises(ValueError):
            ColumnString.concat(*args)


def test_shim_string_functions_compile():
    # syntax-only: the members of chgpu::ColumnString as a driver uses them (no GPU, no library)
    src = os.path.join(REPO, "tests", "string_functions_shim_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
