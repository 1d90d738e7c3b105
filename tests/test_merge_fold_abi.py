"""The C ABI of the folding merges without a GPU: the three entry points are declared, bound and exported, the enum and the cited files are
in the header, NULL and malformed arguments answer with a message in front of the device (a wrong sign / is_deleted type, a Float
value or version column, nine keys, bad offsets, no runs), the Python layer rejects bad input before it touches the library, the shim's
four transforms compile, and the fold of merge_fold_host.h runs under a sanitizer as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOLS = ("chgpu_merge_replacing", "chgpu_merge_collapsing", "chgpu_merge_folding")


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


def _expect(K, rc, code, word):
    assert rc == code
    with pytest.raises(K.ChgpuError) as e:
        K.check(rc)
    assert e.value.code == code and word in str(e.value), str(e.value)


@pytest.fixture()
def call(K):
    """-> (replacing, collapsing, folding) over one Int64 key column of 4 rows in 2 runs; keyword arguments replace the defaults"""
    L = K.lib()
    # a context is looked at first and never dereferenced in the checks in front of the device
    ctx_bytes = C.create_string_buffer(1 << 16)   # zeroes, alive for as long as `fake` is used
    fake = C.c_void_p(C.addressof(ctx_bytes))
    key = _col(K.I64, 4)
    base = dict(ctx=fake, cols=(C.c_void_p * 9)(*([C.addressof(key)] * 9)), desc=(C.c_int32 * 9)(*([0] * 9)), hint=(C.c_int32 * 9)(*([1] * 9)), n_keys=1,
                offs=(C.c_uint64 * 3)(0, 2, 4), n_runs=2, flags=0)
    keep = [key, ctx_bytes]

    def prefix(kw):
        a = dict(base, **{k: v for k, v in kw.items() if k in base})
        return [a["ctx"], a["cols"], a["desc"], a["hint"], a["n_keys"], a["offs"], a["n_runs"], a["flags"]]

    def ptr(c):
        if c is None:
            return None
        keep.append(c)
        return C.addressof(c)

    def replacing(version=None, is_deleted=None, cleanup=0, out=True, **kw):
        o = C.c_void_p()
        rc = L.chgpu_merge_replacing(*prefix(kw), ptr(version), ptr(is_deleted), cleanup, C.byref(o) if out else None)
        assert not o.value
        return rc

    def collapsing(sign=None, out=True, **kw):
        o = C.c_void_p()
        rc = L.chgpu_merge_collapsing(*prefix(kw), ptr(sign), C.byref(o) if out else None)
        assert not o.value
        return rc

    def folding(values=(), kinds=(), drop_zero=0, first=True, last=True, res=True, **kw):
        n = len(values) if values is not None else len(kinds)
        f, la = C.c_void_p(), C.c_void_p()
        r = (C.c_void_p * max(n, 1))()
        rc = L.chgpu_merge_folding(*prefix(kw), (C.c_void_p * max(n, 1))(*[ptr(v) for v in values]) if values is not None else None,
                                   (C.c_int32 * max(n, 1))(*kinds) if kinds is not None else None, kw.get("n_values", n), drop_zero,
                                   C.byref(f) if first else None, C.byref(la) if last else None, r if res else None)
        assert not f.value and not la.value and not any(r)
        return rc

    return replacing, collapsing, folding


def test_entry_points_are_declared_bound_and_exported(K):
    for name in SYMBOLS:
        assert name in K.declared_symbols() and name in K.SIGNATURES
        assert getattr(K.lib(), name)
    assert K.lib().chgpu_abi_version() == 1


def test_enum_and_citations_are_in_the_header(K):
    header = open(K.HEADER_PATH).read()
    assert "enum { CHGPU_FOLD_SUM = 0, CHGPU_FOLD_MIN = 1, CHGPU_FOLD_MAX = 2 };" in header
    assert (K.FOLD_SUM, K.FOLD_MIN, K.FOLD_MAX) == (0, 1, 2)
    for name in ("ReplacingSorted", "CollapsingSorted", "SummingSorted", "AggregatingSorted"):
        assert f"src/Processors/Merges/Algorithms/{name}Algorithm.cpp" in header
    for word in ("hasEqualSortColumnsWith", "sumWithOverflow", "first_negative", "last_positive", "last_is_positive", "drop_zero", "cleanup"):
        assert word in header
    kernels = open(os.path.join(REPO, "clickhouse_amd", "csrc", "merge_fold_kernels.hip")).read()
    assert "src/Processors/Merges/Algorithms/{ReplacingSorted,CollapsingSorted,SummingSorted,AggregatingSorted}Algorithm.cpp" in kernels


def test_python_mirrors_the_fold_geometry():
    from clickhouse_amd import merge_fold, merge_sorted
    host = open(os.path.join(REPO, "clickhouse_amd", "csrc", "merge_fold_host.h")).read()
    assert "FOLD_TILE = MRG_TILE;" in host and merge_fold.TILE == merge_sorted.TILE
    assert merge_fold.MAX_VALUES == int(re.search(r"FOLD_MAX_VALUES = (\d+);", host).group(1))


def test_null_arguments_are_bad_arguments(K, call):
    replacing, collapsing, folding = call
    sign = _col(K.I8, 4)
    bad = K.ERR_BAD_ARGUMENTS
    for kw in (dict(ctx=None), dict(cols=None), dict(desc=None), dict(hint=None), dict(offs=None)):
        _expect(K, replacing(**kw), bad, "NULL")
        _expect(K, collapsing(sign=sign, **kw), bad, "NULL")
        _expect(K, folding(**kw), bad, "NULL")
    _expect(K, replacing(out=False), bad, "NULL")
    _expect(K, collapsing(sign=sign, out=False), bad, "NULL")
    _expect(K, collapsing(sign=None), bad, "NULL")
    _expect(K, folding(first=False), bad, "NULL")
    _expect(K, folding(last=False), bad, "NULL")
    value = _col(K.I64, 4)
    _expect(K, folding(values=[value], kinds=[0], res=False), bad, "NULL")
    _expect(K, folding(values=None, kinds=[0], n_values=1), bad, "NULL")
    _expect(K, folding(values=[value], kinds=None), bad, "NULL")
    _expect(K, folding(values=[None], kinds=[0]), bad, "value column 0 is NULL")
    _expect(K, replacing(cols=(C.c_void_p * 1)(None)), bad, "NULL")     # key column 0


def test_key_counts_offsets_runs_and_flags(K, call):
    bad = K.ERR_BAD_ARGUMENTS
    sign = _col(K.I8, 4)
    for f in (call[0], lambda **kw: call[1](sign=sign, **kw), call[2]):
        _expect(K, f(n_keys=0), bad, "key columns")
        _expect(K, f(n_keys=9), bad, "key columns")
        _expect(K, f(offs=(C.c_uint64 * 3)(1, 2, 4)), bad, "start at 0")
        _expect(K, f(offs=(C.c_uint64 * 3)(0, 5, 4)), bad, "decrease")
        _expect(K, f(offs=(C.c_uint64 * 1)(0), n_runs=0), K.ERR_SIZES_MISMATCH, "rows")      # the keys have 4 rows
        _expect(K, f(flags=2), bad, "flag")
        _expect(K, f(offs=(C.c_uint64 * 2)(0, 2**32), n_runs=1), K.ERR_NOT_IMPLEMENTED, "2^32")
        _expect(K, f(offs=(C.c_uint64 * 3)(0, 2, 5)), K.ERR_SIZES_MISMATCH, "rows")
    empty = _col(K.I64, 0)
    _expect(K, call[0](cols=(C.c_void_p * 1)(C.addressof(empty)), offs=(C.c_uint64 * 1)(0), n_runs=0), bad, "no runs")


def test_argument_columns_are_checked_in_front_of_the_device(K, call):
    replacing, collapsing, folding = call
    bad, missing = K.ERR_BAD_ARGUMENTS, K.ERR_NOT_IMPLEMENTED
    _expect(K, collapsing(sign=_col(K.U8, 4)), bad, "sign")
    _expect(K, collapsing(sign=_col(K.I16, 4)), bad, "Int8")
    _expect(K, collapsing(sign=_col(K.I8, 5)), K.ERR_SIZES_MISMATCH, "sign")
    _expect(K, replacing(version=_col(K.F64, 4)), missing, "Float")
    _expect(K, replacing(version=_col(K.F32, 4)), missing, "Float")
    _expect(K, replacing(version=_col(99, 4)), bad, "unknown type")
    _expect(K, replacing(version=_col(K.U64, 3)), K.ERR_SIZES_MISMATCH, "version")
    _expect(K, replacing(is_deleted=_col(K.U8, 4)), missing, "without a version")
    _expect(K, replacing(version=_col(K.U64, 4), is_deleted=_col(K.I8, 4)), bad, "is_deleted")
    _expect(K, replacing(version=_col(K.U64, 4), is_deleted=_col(K.U8, 2)), K.ERR_SIZES_MISMATCH, "is_deleted")
    _expect(K, folding(values=[_col(K.I64, 4), _col(K.F64, 4)], kinds=[0, 0]), missing, "value column 1 is a Float")
    _expect(K, folding(values=[_col(K.F32, 4)], kinds=[1]), missing, "Float")
    _expect(K, folding(values=[_col(K.I64, 4)], kinds=[3]), bad, "fold kind")
    _expect(K, folding(values=[_col(K.I64, 4)], kinds=[-1]), bad, "fold kind")
    _expect(K, folding(values=[_col(77, 4)], kinds=[0]), bad, "unknown type")
    _expect(K, folding(values=[_col(K.I8, 6)], kinds=[0]), K.ERR_SIZES_MISMATCH, "value column 0")
    _expect(K, folding(values=[_col(K.I8, 4)] * 9, kinds=[0] * 9), missing, "at most 8")


def test_python_rejects_bad_input_before_the_library(K, monkeypatch):
    import clickhouse_amd
    from clickhouse_amd import merge_fold as M
    from clickhouse_amd import merge_sorted
    from clickhouse_amd.lowcardinality import ColumnString
    for name in ("replacing_merge", "collapsing_merge", "summing_merge", "aggregating_merge", "replacing_merge_rows", "collapsing_merge_rows",
                 "summing_merge_rows", "aggregating_merge_rows"):
        assert getattr(clickhouse_amd, name) is getattr(M, name)

    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(K, "lib", touched)
    monkeypatch.setattr(M, "Context", touched)
    monkeypatch.setattr(merge_sorted, "Context", touched)
    s = ColumnString.__new__(ColumnString)
    key = np.arange(4, dtype=np.int64)
    i8, u8, f64 = np.ones(4, dtype=np.int8), np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.float64)
    asc = [(0, False, 1)]
    with pytest.raises(TypeError):
        M.collapsing_merge_rows([s], asc, [0, 4], i8)
    with pytest.raises(TypeError):
        M.collapsing_merge_rows([key], asc, [0, 4], u8)              # the sign is Int8
    with pytest.raises(TypeError):
        M.collapsing_merge_rows([key], asc, [0, 4], key)
    with pytest.raises(TypeError):
        M.collapsing_merge([[key, i8, s]], asc, 1)                    # a carried String column
    with pytest.raises(TypeError):
        M.collapsing_merge([[key, u8]], asc, 1)
    with pytest.raises(ValueError):
        M.collapsing_merge([[key, i8]], asc, 2)
    with pytest.raises(TypeError):
        M.replacing_merge_rows([key], asc, [0, 4], version=f64)
    with pytest.raises(TypeError):
        M.replacing_merge_rows([key], asc, [0, 4], version=s)
    with pytest.raises(TypeError):
        M.replacing_merge_rows([key], asc, [0, 4], version=key, is_deleted=i8)
    with pytest.raises(ValueError):
        M.replacing_merge_rows([key], asc, [0, 4], is_deleted=u8)
    with pytest.raises(TypeError):
        M.replacing_merge([[key, f64]], asc, version=1)
    with pytest.raises(ValueError):
        M.replacing_merge([[key, key]], asc, version=5)
    with pytest.raises(ValueError):
        M.replacing_merge([[key, u8]], asc, is_deleted=1)
    with pytest.raises(TypeError):
        M.summing_merge_rows([key], asc, [0, 4], [f64])
    with pytest.raises(TypeError):
        M.aggregating_merge_rows([key], asc, [0, 4], [key, s], ["sum", "min"])
    with pytest.raises(ValueError):
        M.aggregating_merge_rows([key], asc, [0, 4], [key], ["avg"])
    with pytest.raises(ValueError):
        M.aggregating_merge_rows([key], asc, [0, 4], [key], ["sum", "min"])
    with pytest.raises(ValueError):
        M.summing_merge_rows([key], asc, [0, 4], [key] * 9)
    with pytest.raises(TypeError):
        M.summing_merge([[key, f64]], asc, [1])
    with pytest.raises(ValueError):
        M.summing_merge([[key, key]], asc, [0])                       # a key column
    with pytest.raises(ValueError):
        M.aggregating_merge([[key, key]], asc, {1: "avg"})
    with pytest.raises(ValueError):
        M.aggregating_merge([[key, key]], asc, {0: "max"})
    with pytest.raises(TypeError):
        M.aggregating_merge([[key, f64]], asc, {1: "max"})
    for bad in ([], [(0, False, 1)] * 9, [(1, False, 1)], [(0, False)], [(0, False, 0)]):
        with pytest.raises(ValueError):
            M.collapsing_merge_rows([key], bad, [0, 4], i8)
        with pytest.raises(ValueError):
            M.replacing_merge([[key]], bad)
        with pytest.raises(ValueError):
            M.summing_merge([[key]], bad)
    for offsets in ([], [1, 4], [0, 3, 2, 4], [0, 3]):
        with pytest.raises(ValueError):
            M.replacing_merge_rows([key], asc, offsets)
    with pytest.raises(ValueError):
        M.replacing_merge([], asc)
    with pytest.raises(ValueError):
        M.summing_merge([[key], [key, key]], asc)


def test_shim_transforms_compile(tmp_path):
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
template <typename Transform>
Chunk run(Transform & merge, std::vector<std::vector<Chunk>> & parts)
{
    for (size_t input = 0; input < parts.size(); ++input)
        for (auto & chunk : parts[input])
            merge.consume(input, std::move(chunk));
    return merge.finish();
}
Chunk final_replacing(ContextPtr ctx, std::vector<std::vector<Chunk>> parts)
{
    // SELECT .. FINAL over ReplacingMergeTree(version, is_deleted) ORDER BY (k, t)
    GpuReplacingSortedTransform merge(ctx, parts.size(), SortDescription{{0, 1, 1}, {1, 1, 1}}, 2, 3, true);
    return run(merge, parts);
}
Chunk final_collapsing(ContextPtr ctx, std::vector<std::vector<Chunk>> parts)
{
    GpuCollapsingSortedTransform merge(ctx, parts.size(), SortDescription{{0, 1, 1}}, 2);
    return run(merge, parts);
}
Chunk final_summing(ContextPtr ctx, std::vector<std::vector<Chunk>> parts)
{
    GpuSummingSortedTransform merge(ctx, parts.size(), SortDescription{{0, -1, 1}}, {1, 2});
    return run(merge, parts);
}
Chunk final_aggregating(ContextPtr ctx, std::vector<std::vector<Chunk>> parts)
{
    GpuAggregatingSortedTransform merge(ctx, parts.size(), SortDescription{{0, 1, 1}}, {{1, CHGPU_FOLD_MAX}, {2, CHGPU_FOLD_SUM}}, {3});
    return run(merge, parts);
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_fold_under_address_and_undefined_sanitizers(tmp_path):
    # states, combine operators, the segmented scan, carries, tail counts, offsets and stores need no device: a stand-alone program with its
    # own main, run as a plain executable
    exe = tmp_path / "merge_fold_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "merge_fold_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "merge_fold_driver OK" in r.stdout, r.stdout + r.stderr
