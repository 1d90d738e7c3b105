"""The C ABI of groupArray / groupArray(N) without a GPU: every entry point is declared, bound and exported, answers a NULL handle with
BAD_ARGUMENTS and a message, the Python class rejects an unknown dtype before it touches the library, the shim's class compiles, and the
host-only parts run under a sanitizer as a stand-alone program (the checks that need a context are in test_gpu_group_array.py)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOLS = ("chgpu_group_array_create", "chgpu_group_array_add_block", "chgpu_group_array_merge", "chgpu_group_array_size",
           "chgpu_group_array_export_pairs", "chgpu_group_array_finalize", "chgpu_group_array_for_keys", "chgpu_group_array_free")


@pytest.fixture(scope="module")
def K():
    from clickhouse_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def _expect_bad(K, rc):
    assert rc == K.ERR_BAD_ARGUMENTS
    with pytest.raises(K.ChgpuError) as e:
        K.check(rc)
    assert e.value.code == K.ERR_BAD_ARGUMENTS and "NULL" in str(e.value)


def test_entry_points_are_declared_bound_and_exported(K):
    for name in SYMBOLS:
        assert name in K.declared_symbols() and name in K.SIGNATURES
        assert getattr(K.lib(), name)
    assert K.lib().chgpu_abi_version() == 1
    header = open(K.HEADER_PATH).read()
    assert "typedef struct chgpu_group_array chgpu_group_array;" in header
    assert "uint64_t max_size, chgpu_group_array ** out" in header


def test_create_rejects_null(K):
    h = C.c_void_p()
    _expect_bad(K, K.lib().chgpu_group_array_create(None, K.U64, K.F64, 0, C.byref(h)))
    _expect_bad(K, K.lib().chgpu_group_array_create(None, K.U64, K.F64, 10, None))


def test_add_block_and_merge_reject_null(K):
    _expect_bad(K, K.lib().chgpu_group_array_add_block(None, None, None, 0, 0, None))
    _expect_bad(K, K.lib().chgpu_group_array_merge(None, None))


def test_size_export_finalize_and_for_keys_reject_null(K):
    n = C.c_uint64(0)
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _expect_bad(K, K.lib().chgpu_group_array_size(None, C.byref(n)))
    _expect_bad(K, K.lib().chgpu_group_array_export_pairs(None, C.byref(a), C.byref(b), C.byref(n)))
    _expect_bad(K, K.lib().chgpu_group_array_finalize(None, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
    _expect_bad(K, K.lib().chgpu_group_array_for_keys(None, None, C.byref(a), C.byref(b)))


def test_free_takes_null(K):
    assert K.lib().chgpu_group_array_free(None) == K.OK


def test_python_class_rejects_an_unknown_dtype_before_the_library(K):
    from clickhouse_amd.group_array import GroupArray
    with pytest.raises(ValueError):
        GroupArray("complex64", "int64", ctx=object())
    with pytest.raises(ValueError):
        GroupArray("uint64", "U3", ctx=object())
    with pytest.raises(ValueError):
        GroupArray(None, "float16", ctx=object())
    with pytest.raises(ValueError):
        GroupArray("uint64", "int64", max_size=-1, ctx=object())
    import clickhouse_amd
    assert clickhouse_amd.GroupArray is GroupArray


def test_shim_class_compiles_next_to_an_aggregator(tmp_path):
    # syntax-only: GpuGroupArray as a driver uses it (no GPU, no library)
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
Chunk drive(ContextPtr ctx, Chunk chunk)
{
    // SELECT k, sum(a), groupArray(x), groupArrayIf(10)(y, c) ... GROUP BY k: columns k, a, x, y, c
    GpuAggregator agg(ctx, CHGPU_U32, {AggregateDescription{CHGPU_AGG_SUM, CHGPU_I64, 1}}, 0);
    GpuGroupArray g_x(ctx, CHGPU_U32, CHGPU_F64), g_y_if(ctx, CHGPU_U32, CHGPU_I16, 10), other(ctx, CHGPU_U32, CHGPU_F64);
    GpuGroupArray without_key(ctx, -1, CHGPU_U8);
    agg.executeOnBlock(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0));
    g_x.add(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0), 2);
    g_y_if.add(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0), 3, std::optional<size_t>(4));
    without_key.add(chunk.columns, 0, chunk.num_rows, std::nullopt, 4);
    g_x.merge(other);
    size_t values = g_x.size() + static_cast<size_t>(g_x.keyType() + g_x.valueType()) + g_y_if.maxSize();
    (void)values;
    Chunk not_final = g_x.convertToBlock(false);
    other.add(not_final.columns, 0, not_final.num_rows, std::optional<size_t>(0), 1);
    Chunk one_row = without_key.convertToBlock();
    (void)one_row;
    Chunk out = agg.convertToBlock();
    GpuColumnArray arrays = g_x.arraysForKeys(*out.columns.at(0));
    out.columns.push_back(arrays.offsets);
    out.columns.push_back(arrays.data);
    out.columns.push_back(g_y_if.arraysForKeys(*out.columns.at(0)).offsets);
    return out;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_host_only_parts_under_address_and_undefined_sanitizers(tmp_path):
    # pass planning, capacity growth, the segmented copy's unit arithmetic and the plan lines need no device: a stand-alone program
    # with its own main, run as a plain executable
    exe = tmp_path / "group_array_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "group_array_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "group_array_driver OK" in r.stdout, r.stdout + r.stderr
