"""The C ABI of the merge of sorted runs without a GPU: the two entry points are declared, bound and exported, the flag is in the header,
NULL arguments and malformed offsets answer BAD_ARGUMENTS with a message, the Python layer rejects String columns and bad descriptions
before it touches the library, the shim's two transforms compile, and the host-only parts run under a sanitizer as a stand-alone program
(the checks that need a context are in test_gpu_merge_sorted.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOLS = ("chgpu_merge_sorted_permutation", "chgpu_is_sorted")


@pytest.fixture(scope="module")
def K():
    from clickhouse_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def _expect_bad(K, rc, word):
    assert rc == K.ERR_BAD_ARGUMENTS
    with pytest.raises(K.ChgpuError) as e:
        K.check(rc)
    assert e.value.code == K.ERR_BAD_ARGUMENTS and word in str(e.value)


def test_entry_points_are_declared_bound_and_exported(K):
    for name in SYMBOLS:
        assert name in K.declared_symbols() and name in K.SIGNATURES
        assert getattr(K.lib(), name)
    assert K.lib().chgpu_abi_version() == 1


def test_flag_and_citations_are_in_the_header(K):
    header = open(K.HEADER_PATH).read()
    assert "enum { CHGPU_MERGE_CHECK_SORTED = 1 };" in header and K.MERGE_CHECK_SORTED == 1
    for cited in ("src/Processors/Merges/Algorithms/MergingSortedAlgorithm.cpp", "src/Core/SortCursor.h",
                  "src/Processors/Transforms/MergeSortingTransform.cpp", "isAlreadySorted", "src/Interpreters/sortBlock.cpp"):
        assert cited in header


def test_python_mirrors_the_tile_geometry():
    from clickhouse_amd import merge_sorted
    host = open(os.path.join(REPO, "clickhouse_amd", "csrc", "merge_host.h")).read()
    threads = int(re.search(r"MRG_THREADS = (\d+);", host).group(1))
    items = int(re.search(r"MRG_ITEMS = (\d+);", host).group(1))
    assert "MRG_TILE = MRG_THREADS * MRG_ITEMS;" in host and merge_sorted.TILE == threads * items
    assert merge_sorted.MAX_KEYS == int(re.search(r"MRG_MAX_KEYS = (\d+);", host).group(1))
    assert merge_sorted.MAX_ROWS == 0xFFFFFFFF and "MRG_MAX_ROWS = 0xFFFFFFFFull;" in host


def test_null_arguments_are_bad_arguments(K):
    L = K.lib()
    out, row = C.c_void_p(), C.c_uint64(0)
    cols = (C.c_void_p * 1)(None)
    desc, hint = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
    offs = (C.c_uint64 * 2)(0, 0)
    _expect_bad(K, L.chgpu_merge_sorted_permutation(None, cols, desc, hint, 1, offs, 1, 0, 0, C.byref(out)), "NULL")
    _expect_bad(K, L.chgpu_merge_sorted_permutation(None, cols, desc, hint, 1, offs, 1, 0, 0, None), "NULL")
    _expect_bad(K, L.chgpu_is_sorted(None, cols, desc, hint, 1, offs, 1, C.byref(row)), "NULL")
    _expect_bad(K, L.chgpu_is_sorted(None, cols, desc, hint, 1, offs, 1, None), "NULL")
    # a context is looked at first and never dereferenced: any non-NULL pointer stands for one in the checks in front of the device
    ctx_bytes = C.create_string_buffer(1 << 16)   # zeroes, alive for as long as `fake` is used
    fake = C.c_void_p(C.addressof(ctx_bytes))
    _expect_bad(K, L.chgpu_merge_sorted_permutation(fake, None, desc, hint, 1, offs, 1, 0, 0, C.byref(out)), "NULL")
    _expect_bad(K, L.chgpu_merge_sorted_permutation(fake, cols, None, hint, 1, offs, 1, 0, 0, C.byref(out)), "NULL")
    _expect_bad(K, L.chgpu_merge_sorted_permutation(fake, cols, desc, None, 1, offs, 1, 0, 0, C.byref(out)), "NULL")
    _expect_bad(K, L.chgpu_merge_sorted_permutation(fake, cols, desc, hint, 1, None, 1, 0, 0, C.byref(out)), "NULL")
    _expect_bad(K, L.chgpu_is_sorted(fake, cols, desc, hint, 1, None, 1, C.byref(row)), "NULL")
    _expect_bad(K, L.chgpu_merge_sorted_permutation(fake, cols, desc, hint, 1, offs, 1, 0, 0, C.byref(out)), "NULL")   # key column 0
    assert not out.value


def test_key_counts_and_malformed_offsets_are_bad_arguments(K):
    L = K.lib()
    out, row = C.c_void_p(), C.c_uint64(0)
    ctx_bytes = C.create_string_buffer(1 << 16)   # zeroes, alive for as long as `fake` is used
    fake = C.c_void_p(C.addressof(ctx_bytes))
    cols = (C.c_void_p * 9)(*([None] * 9))
    desc, hint = (C.c_int32 * 9)(*([0] * 9)), (C.c_int32 * 9)(*([1] * 9))
    offs = (C.c_uint64 * 3)(0, 2, 4)
    _expect_bad(K, L.chgpu_merge_sorted_permutation(fake, cols, desc, hint, 0, offs, 2, 0, 0, C.byref(out)), "key columns")
    _expect_bad(K, L.chgpu_merge_sorted_permutation(fake, cols, desc, hint, 9, offs, 2, 0, 0, C.byref(out)), "key columns")
    _expect_bad(K, L.chgpu_is_sorted(fake, cols, desc, hint, 9, offs, 2, C.byref(row)), "key columns")
    late = (C.c_uint64 * 3)(1, 2, 4)
    _expect_bad(K, L.chgpu_merge_sorted_permutation(fake, cols, desc, hint, 1, late, 2, 0, 0, C.byref(out)), "start at 0")
    _expect_bad(K, L.chgpu_is_sorted(fake, cols, desc, hint, 1, late, 2, C.byref(row)), "start at 0")
    down = (C.c_uint64 * 4)(0, 5, 4, 9)
    _expect_bad(K, L.chgpu_merge_sorted_permutation(fake, cols, desc, hint, 1, down, 3, 0, 0, C.byref(out)), "decrease")
    _expect_bad(K, L.chgpu_is_sorted(fake, cols, desc, hint, 1, down, 3, C.byref(row)), "decrease")
    wide = (C.c_uint64 * 2)(0, 2**32)
    rc = L.chgpu_merge_sorted_permutation(fake, cols, desc, hint, 1, wide, 1, 0, 0, C.byref(out))
    assert rc == K.ERR_NOT_IMPLEMENTED and b"2^32" in L.chgpu_last_error()
    assert not out.value


def test_python_rejects_strings_and_bad_descriptions_before_the_library(K, monkeypatch):
    import clickhouse_amd
    from clickhouse_amd import merge_sorted as M
    from clickhouse_amd.lowcardinality import ColumnString
    assert clickhouse_amd.merge_sorted_permutation is M.merge_sorted_permutation and clickhouse_amd.MergeSorting is M.MergeSorting
    assert clickhouse_amd.is_sorted is M.is_sorted and clickhouse_amd.merge_sorted_blocks is M.merge_sorted_blocks

    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(K, "lib", touched)
    monkeypatch.setattr(M, "Context", touched)
    s = ColumnString.__new__(ColumnString)   # no device behind it: the type alone must be enough
    ok = np.arange(4, dtype=np.int64)
    with pytest.raises(TypeError):
        M.is_sorted([s], [(0, False, 1)])
    with pytest.raises(TypeError):
        M.merge_sorted_permutation([ok, s], [(0, False, 1)], [0, 4])
    with pytest.raises(TypeError):
        M.merge_sorted_blocks([[ok, s]], [(0, False, 1)])      # a carried String column
    with pytest.raises(TypeError):
        M.merge_sorted_blocks([[ok], [np.array(["a", "b"])]], [(0, False, 1)])
    with pytest.raises(TypeError):
        M.MergeSorting([(0, False, 1)]).add_block([ok, s])
    with pytest.raises(TypeError):
        M.is_sorted([np.zeros(4, dtype=np.float16)], [(0, False, 1)])
    for bad in ([], [(0, False, 1)] * 9, [(1, False, 1)], [(-1, False, 1)], [(0, False)], [(0, False, 0)], [(0.5, False, 1)]):
        with pytest.raises(ValueError):
            M.merge_sorted_permutation([ok], bad, [0, 4])
        with pytest.raises(ValueError):
            M.MergeSorting(bad).add_block([ok])
    for offsets in ([], [1, 4], [0, 3, 2, 4], [0, 3], [0, 5]):
        with pytest.raises(ValueError):
            M.merge_sorted_permutation([ok], [(0, False, 1)], offsets)
    with pytest.raises(ValueError):
        M.merge_sorted_permutation([ok], [(0, False, 1)], [0, 4], limit=-1)
    with pytest.raises(ValueError):
        M.merge_sorted_permutation([ok, np.zeros(5, dtype=np.int8)], [(0, False, 1), (1, False, 1)], [0, 4])
    with pytest.raises(ValueError):
        M.merge_sorted_blocks([], [(0, False, 1)])
    with pytest.raises(ValueError):
        M.merge_sorted_blocks([[ok], [ok, ok]], [(0, False, 1)])
    with pytest.raises(ValueError):
        M.MergeSorting([(0, False, 1)], limit=-1)


def test_shim_transforms_compile(tmp_path):
    # syntax-only: the two transforms as a driver uses them (no GPU, no library)
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
Chunk merge_streams(ContextPtr ctx, std::vector<std::vector<Chunk>> sorted_streams)
{
    // SELECT .. ORDER BY k DESC, t LIMIT 10 over three sorted inputs (the shards of a Distributed table)
    SortDescription description{{0, -1, 1}, {1, 1, 1}};
    GpuMergingSortedTransform merging(ctx, sorted_streams.size(), description, 10);
    for (size_t input = 0; input < sorted_streams.size(); ++input)
        for (auto & chunk : sorted_streams[input])
            merging.consume(input, std::move(chunk));
    return merging.finish();
}
Chunk sort_stream(ContextPtr ctx, std::vector<Chunk> chunks)
{
    GpuMergeSortingTransform sorting(ctx, SortDescription{{1, 1, -1}});
    for (auto & chunk : chunks)
        sorting.consume(std::move(chunk));
    return sorting.generate();
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_host_only_parts_under_address_and_undefined_sanitizers(tmp_path):
    # offset validation, the round run-lists, the tile-to-pair table, the merge-path search, the tree replayed tile by tile and the plan
    # need no device: a stand-alone program with its own main, run as a plain executable
    exe = tmp_path / "merge_sorted_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "merge_sorted_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "merge_sorted_driver OK" in r.stdout, r.stdout + r.stderr
