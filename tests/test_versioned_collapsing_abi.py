"""The C ABI of the VersionedCollapsing merge without a GPU: the entry point is declared, bound and exported, the cited file and the words
of its contract are in the header, NULL and malformed arguments answer with a message in front of the device and write nothing to the
outputs, the Python layer rejects bad input before it touches the library, the shim's transform compiles, and the scans and the survive
rule of merge_versioned_host.h run under a sanitizer as a stand-alone program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOL = "chgpu_merge_versioned_collapsing"
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


def _expect(K, rc, code, word):
    assert rc == code
    with pytest.raises(K.ChgpuError) as e:
        K.check(rc)
    assert e.value.code == code and word in str(e.value), str(e.value)


@pytest.fixture()
def call(K):
    """the entry point over (Int64 key, UInt32 version) of 4 rows in 2 runs; keyword arguments replace the defaults.  Every call checks
    that neither output was written."""
    L = K.lib()
    # a context is looked at first and never dereferenced in the checks in front of the device
    ctx_bytes = C.create_string_buffer(1 << 16)   # zeroes, alive for as long as `fake` is used
    fake = C.c_void_p(C.addressof(ctx_bytes))
    key, version = _col(K.I64, 4), _col(K.U32, 4)
    base = dict(ctx=fake, cols=(C.c_void_p * 9)(C.addressof(key), *([C.addressof(version)] * 8)), desc=(C.c_int32 * 9)(*([0] * 9)),
                hint=(C.c_int32 * 9)(*([1] * 9)), n_keys=2, offs=(C.c_uint64 * 3)(0, 2, 4), n_runs=2, flags=0)
    keep = [key, version, ctx_bytes]

    def versioned(sign=None, out=True, balance=True, **kw):
        a = dict(base, **kw)
        if sign is not None:
            keep.append(sign)
        o, b = C.c_void_p(), C.c_uint64(UNTOUCHED)
        rc = L.chgpu_merge_versioned_collapsing(a["ctx"], a["cols"], a["desc"], a["hint"], a["n_keys"], a["offs"], a["n_runs"], a["flags"],
                                                C.addressof(sign) if sign is not None else None, C.byref(o) if out else None, C.byref(b) if balance else None)
        assert not o.value and b.value == UNTOUCHED
        return rc

    return versioned


def test_entry_point_is_declared_bound_and_exported(K):
    assert SYMBOL in K.declared_symbols() and SYMBOL in K.SIGNATURES
    assert getattr(K.lib(), SYMBOL)
    assert getattr(C.CDLL(K.LIB_PATH), SYMBOL)
    assert len(K.SIGNATURES[SYMBOL][1]) == 11


def test_citation_and_contract_words_are_in_the_header(K):
    header = open(K.HEADER_PATH).read()
    assert "src/Processors/Merges/Algorithms/VersionedCollapsingAlgorithm.cpp" in header
    for word in ("sign_in_queue", "max_balance", "unbounded", "max_rows_in_queue"):
        assert word in header
    assert "VersionedCollapsing have no" not in " ".join(header.split())       # the Collapsing paragraph no longer disclaims it
    for name in ("merge_versioned_kernels.hip", "merge_versioned_host.h"):
        text = open(os.path.join(REPO, "clickhouse_amd", "csrc", name)).read()
        assert "src/Processors/Merges/Algorithms/VersionedCollapsingAlgorithm.cpp" in text
    makefile = open(os.path.join(REPO, "clickhouse_amd", "csrc", "Makefile")).read()
    assert "merge_versioned_kernels.hip" in makefile and "merge_versioned_host.h" in makefile


def test_null_arguments_are_bad_arguments(K, call):
    sign = _col(K.I8, 4)
    bad = K.ERR_BAD_ARGUMENTS
    for kw in (dict(ctx=None), dict(cols=None), dict(desc=None), dict(hint=None), dict(offs=None)):
        _expect(K, call(sign=sign, **kw), bad, "NULL")
    _expect(K, call(sign=None), bad, "NULL")
    _expect(K, call(sign=sign, out=False), bad, "NULL")
    _expect(K, call(sign=None, balance=False), bad, "NULL")
    _expect(K, call(sign=sign, cols=(C.c_void_p * 2)(None, None)), bad, "NULL")     # key column 0


def test_key_counts_offsets_runs_and_flags(K, call):
    bad = K.ERR_BAD_ARGUMENTS
    sign = _col(K.I8, 4)
    for balance in (True, False):
        def f(**kw):
            return call(sign=sign, balance=balance, **kw)
        _expect(K, f(n_keys=0), bad, "key columns")
        _expect(K, f(n_keys=9), bad, "key columns")
        _expect(K, f(offs=(C.c_uint64 * 3)(1, 2, 4)), bad, "start at 0")
        _expect(K, f(offs=(C.c_uint64 * 3)(0, 5, 4)), bad, "decrease")
        _expect(K, f(offs=(C.c_uint64 * 1)(0), n_runs=0), K.ERR_SIZES_MISMATCH, "rows")      # the keys have 4 rows
        _expect(K, f(flags=2), bad, "flag")
        _expect(K, f(offs=(C.c_uint64 * 2)(0, 2**32), n_runs=1), K.ERR_NOT_IMPLEMENTED, "2^32")
        _expect(K, f(offs=(C.c_uint64 * 3)(0, 2, 5)), K.ERR_SIZES_MISMATCH, "rows")
    empty = _col(K.I64, 0)
    _expect(K, call(sign=_col(K.I8, 0), cols=(C.c_void_p * 1)(C.addressof(empty)), n_keys=1, offs=(C.c_uint64 * 1)(0), n_runs=0), bad, "no runs")


def test_the_sign_column_is_checked_in_front_of_the_device(K, call):
    bad = K.ERR_BAD_ARGUMENTS
    _expect(K, call(sign=_col(K.U8, 4)), bad, "sign")
    _expect(K, call(sign=_col(K.I16, 4)), bad, "Int8")
    _expect(K, call(sign=_col(K.F32, 4)), bad, "Int8")
    _expect(K, call(sign=_col(K.I8, 5)), K.ERR_SIZES_MISMATCH, "sign")
    _expect(K, call(sign=_col(K.I8, 3)), K.ERR_SIZES_MISMATCH, "sign")


def test_python_rejects_bad_input_before_the_library(K, monkeypatch):
    import clickhouse_amd
    from clickhouse_amd import merge_fold as M
    from clickhouse_amd import merge_sorted
    from clickhouse_amd.lowcardinality import ColumnString
    for name in ("versioned_collapsing_merge", "versioned_collapsing_merge_rows"):
        assert getattr(clickhouse_amd, name) is getattr(M, name)

    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(K, "lib", touched)
    monkeypatch.setattr(M, "Context", touched)
    monkeypatch.setattr(merge_sorted, "Context", touched)
    s = ColumnString.__new__(ColumnString)
    key, version = np.arange(4, dtype=np.int64), np.zeros(4, dtype=np.uint32)
    i8, u8, f64 = np.ones(4, dtype=np.int8), np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.float64)
    spec = [(0, False, 1), (1, False, 1)]
    with pytest.raises(TypeError):
        M.versioned_collapsing_merge_rows([s, version], spec, [0, 4], i8)
    for sign in (u8, key, f64, s):
        with pytest.raises(TypeError):
            M.versioned_collapsing_merge_rows([key, version], spec, [0, 4], sign)      # the sign is Int8
    with pytest.raises(TypeError):
        M.versioned_collapsing_merge([[key, version, i8, s]], spec, 2)                  # a carried String column
    with pytest.raises(TypeError):
        M.versioned_collapsing_merge([[key, version, u8]], spec, 2)
    for position in (3, -1, 1.5, None):
        with pytest.raises(ValueError):
            M.versioned_collapsing_merge([[key, version, i8]], spec, position)
    with pytest.raises(ValueError):
        M.versioned_collapsing_merge([[key, version, i8], [key, version]], spec, 2)     # ragged blocks
    with pytest.raises(ValueError):
        M.versioned_collapsing_merge([], spec, 2)
    for bad in ([], [(0, False, 1)] * 9, [(2, False, 1)], [(0, False)], [(0, False, 0)]):
        with pytest.raises(ValueError):
            M.versioned_collapsing_merge_rows([key, version], bad, [0, 4], i8)
        with pytest.raises(ValueError):
            M.versioned_collapsing_merge([[key, version]], bad, 1)
    for offsets in ([], [1, 4], [0, 3, 2, 4], [0, 3]):
        with pytest.raises(ValueError):
            M.versioned_collapsing_merge_rows([key, version], spec, offsets, i8)


def test_shim_transform_compiles(tmp_path):
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
Chunk final_versioned_collapsing(ContextPtr ctx, std::vector<std::vector<Chunk>> parts, uint64_t max_rows_in_queue, bool & same_as_reference)
{
    // SELECT .. FINAL over VersionedCollapsingMergeTree(sign, version) ORDER BY k: the description ends with the version
    GpuVersionedCollapsingSortedTransform merge(ctx, parts.size(), SortDescription{{0, 1, 1}, {2, 1, 1}}, 1);
    for (size_t input = 0; input < parts.size(); ++input)
        for (auto & chunk : parts[input])
            merge.consume(input, std::move(chunk));
    Chunk out = merge.finish();
    same_as_reference = merge.maxBalance() < max_rows_in_queue;
    return out;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_scans_under_address_and_undefined_sanitizers(tmp_path):
    # states, combines, the survive rule, carries, masks, offsets and stores need no device: a stand-alone program with its own main, run
    # as a plain executable
    exe = tmp_path / "merge_versioned_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "merge_versioned_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "merge_versioned_driver OK" in r.stdout, r.stdout + r.stderr
