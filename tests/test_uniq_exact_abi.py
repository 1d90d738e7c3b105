"""The C ABI of uniqExact / count(DISTINCT) without a GPU: every entry point is declared, bound and exported, answers a NULL handle with
BAD_ARGUMENTS and a message, the Python class rejects an unknown dtype before it touches the library, the shim's class compiles, and
the host-only parts run under a sanitizer (the checks that need a context are in test_gpu_uniq_exact.py)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOLS = ("chgpu_uniq_create", "chgpu_uniq_add_block", "chgpu_uniq_merge", "chgpu_uniq_size", "chgpu_uniq_export_pairs", "chgpu_uniq_finalize",
           "chgpu_uniq_counts_for_keys", "chgpu_uniq_free")


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


def test_create_rejects_null(K):
    h = C.c_void_p()
    _expect_bad(K, K.lib().chgpu_uniq_create(None, K.U64, K.U64, 0, C.byref(h)))
    _expect_bad(K, K.lib().chgpu_uniq_create(None, K.U64, K.U64, 0, None))


def test_add_block_and_merge_reject_null(K):
    _expect_bad(K, K.lib().chgpu_uniq_add_block(None, None, None, 0, 0, None))
    _expect_bad(K, K.lib().chgpu_uniq_merge(None, None))


def test_size_export_finalize_and_counts_reject_null(K):
    n = C.c_uint64(0)
    a, b = C.c_void_p(), C.c_void_p()
    _expect_bad(K, K.lib().chgpu_uniq_size(None, C.byref(n)))
    _expect_bad(K, K.lib().chgpu_uniq_export_pairs(None, C.byref(a), C.byref(b), C.byref(n)))
    _expect_bad(K, K.lib().chgpu_uniq_finalize(None, C.byref(a), C.byref(b), C.byref(n)))
    _expect_bad(K, K.lib().chgpu_uniq_counts_for_keys(None, None, C.byref(a)))


def test_free_takes_null(K):
    assert K.lib().chgpu_uniq_free(None) == K.OK


def test_python_class_rejects_an_unknown_dtype_before_the_library(K):
    from clickhouse_amd.uniq import UniqExact
    with pytest.raises(ValueError):
        UniqExact("complex64", "int64", ctx=object())
    with pytest.raises(ValueError):
        UniqExact("uint64", "U3", ctx=object())
    with pytest.raises(ValueError):
        UniqExact(None, "float16", ctx=object())


def test_the_pair_operators_keep_their_public_method_names():
    # the two classes share a base (clickhouse_amd/_pairs.py); what a caller sees of either is this and no more
    from clickhouse_amd.quantile import QuantileExact
    from clickhouse_amd.uniq import UniqExact
    shared = {"add_block", "close", "export_pairs", "finalize", "finalize_columns", "merge"}
    public = lambda cls: {n for n in dir(cls) if not n.startswith("_")}
    assert public(UniqExact) == shared | {"export_pair_columns", "counts_for_keys", "counts_for_keys_column"}
    assert public(QuantileExact) == shared | {"export_pairs_columns", "quantiles_for_keys", "quantiles_for_keys_column"}
    for cls in (UniqExact, QuantileExact):
        assert callable(cls.__len__) and callable(cls.__del__) and all(callable(getattr(cls, n)) for n in public(cls))


def test_shim_class_compiles_next_to_an_aggregator(tmp_path):
    # syntax-only: GpuUniqExact as a driver uses it (no GPU, no library)
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
Chunk drive(ContextPtr ctx, Chunk chunk)
{
    // SELECT k, sum(a), count(DISTINCT x), uniqExactIf(y, c) ... GROUP BY k: columns k, a, x, y, c
    GpuAggregator agg(ctx, CHGPU_U32, {AggregateDescription{CHGPU_AGG_SUM, CHGPU_I64, 1}}, 0);
    GpuUniqExact distinct_x(ctx, CHGPU_U32, CHGPU_F64), distinct_y_if(ctx, CHGPU_U32, CHGPU_I16, 1000), other(ctx, CHGPU_U32, CHGPU_F64);
    GpuUniqExact without_key(ctx, -1, CHGPU_U8);
    agg.executeOnBlock(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0));
    distinct_x.add(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0), 2);
    distinct_y_if.add(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0), 3, std::optional<size_t>(4));
    without_key.add(chunk.columns, 0, chunk.num_rows, std::nullopt, 4);
    distinct_x.merge(other);
    size_t pairs = distinct_x.size() + static_cast<size_t>(distinct_x.keyType() + distinct_x.valueType());
    (void)pairs;
    Chunk not_final = distinct_x.convertToBlock(false);
    other.add(not_final.columns, 0, not_final.num_rows, std::optional<size_t>(0), 1);
    Chunk one_row = without_key.convertToBlock();
    (void)one_row;
    Chunk out = agg.convertToBlock();
    out.columns.push_back(distinct_x.countsForKeys(*out.columns.at(0)));
    out.columns.push_back(distinct_y_if.countsForKeys(*out.columns.at(0)));
    return out;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_host_only_parts_under_address_and_undefined_sanitizers(tmp_path):
    # geometry, row checks and the plan line need no device: a stand-alone program with its own main
    exe = tmp_path / "uniq_exact_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "uniq_exact_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "uniq_exact_driver OK" in r.stdout, r.stdout + r.stderr
