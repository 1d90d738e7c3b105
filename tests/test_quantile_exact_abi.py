"""The C ABI of quantileExact / quantilesExact / medianExact without a GPU: every entry point is declared, bound and exported, answers a
NULL handle with BAD_ARGUMENTS and a message, the Python class rejects an unknown dtype before it touches the library, the shim's
class compiles, and the host-only parts run under a sanitizer as a stand-alone program (the checks that need a context are in
test_gpu_quantile_exact.py)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOLS = ("chgpu_quantile_create", "chgpu_quantile_add_block", "chgpu_quantile_merge", "chgpu_quantile_size", "chgpu_quantile_export_pairs",
           "chgpu_quantile_finalize", "chgpu_quantile_for_keys", "chgpu_quantile_free")


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
    for name, value in (("CHGPU_QUANTILE_EXACT", K.QUANTILE_EXACT), ("CHGPU_QUANTILE_EXACT_LOW", K.QUANTILE_EXACT_LOW),
                        ("CHGPU_QUANTILE_EXACT_HIGH", K.QUANTILE_EXACT_HIGH)):
        assert f"{name} = {value}" in header
    assert f"#define CHGPU_QUANTILE_MAX_LEVELS {K.QUANTILE_MAX_LEVELS}" in header


def test_create_rejects_null(K):
    h = C.c_void_p()
    _expect_bad(K, K.lib().chgpu_quantile_create(None, K.U64, K.F64, C.byref(h)))
    _expect_bad(K, K.lib().chgpu_quantile_create(None, K.U64, K.F64, None))


def test_add_block_and_merge_reject_null(K):
    _expect_bad(K, K.lib().chgpu_quantile_add_block(None, None, None, 0, 0, None))
    _expect_bad(K, K.lib().chgpu_quantile_merge(None, None))


def test_size_export_finalize_and_for_keys_reject_null(K):
    n = C.c_uint64(0)
    a, b = C.c_void_p(), C.c_void_p()
    levels = (C.c_double * 1)(0.5)
    res = (C.c_void_p * 1)()
    _expect_bad(K, K.lib().chgpu_quantile_size(None, C.byref(n)))
    _expect_bad(K, K.lib().chgpu_quantile_export_pairs(None, C.byref(a), C.byref(b), C.byref(n)))
    _expect_bad(K, K.lib().chgpu_quantile_finalize(None, K.QUANTILE_EXACT, 1, levels, C.byref(a), res, C.byref(n)))
    _expect_bad(K, K.lib().chgpu_quantile_for_keys(None, K.QUANTILE_EXACT, 1, levels, None, res))


def test_free_takes_null(K):
    assert K.lib().chgpu_quantile_free(None) == K.OK


def test_python_class_rejects_an_unknown_dtype_before_the_library(K):
    from clickhouse_amd.quantile import QuantileExact
    with pytest.raises(ValueError):
        QuantileExact("complex64", "int64", ctx=object())
    with pytest.raises(ValueError):
        QuantileExact("uint64", "U3", ctx=object())
    with pytest.raises(ValueError):
        QuantileExact(None, "float16", ctx=object())
    import clickhouse_amd
    assert clickhouse_amd.QuantileExact is QuantileExact


def test_shim_class_compiles_next_to_an_aggregator(tmp_path):
    # syntax-only: GpuQuantileExact as a driver uses it (no GPU, no library)
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
Chunk drive(ContextPtr ctx, Chunk chunk)
{
    // SELECT k, sum(a), quantilesExact(0.5, 0.9, 0.99)(x), quantileExactLowIf(0.5)(y, c) ... GROUP BY k: columns k, a, x, y, c
    GpuAggregator agg(ctx, CHGPU_U32, {AggregateDescription{CHGPU_AGG_SUM, CHGPU_I64, 1}}, 0);
    GpuQuantileExact q_x(ctx, CHGPU_U32, CHGPU_F64), q_y_if(ctx, CHGPU_U32, CHGPU_I16), other(ctx, CHGPU_U32, CHGPU_F64);
    GpuQuantileExact without_key(ctx, -1, CHGPU_U8);
    agg.executeOnBlock(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0));
    q_x.add(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0), 2);
    q_y_if.add(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0), 3, std::optional<size_t>(4));
    without_key.add(chunk.columns, 0, chunk.num_rows, std::nullopt, 4);
    q_x.merge(other);
    size_t values = q_x.size() + static_cast<size_t>(q_x.keyType() + q_x.valueType());
    (void)values;
    const std::vector<double> levels{0.5, 0.9, 0.99};
    Chunk not_final = q_x.convertToBlock(levels, CHGPU_QUANTILE_EXACT, false);
    other.add(not_final.columns, 0, not_final.num_rows, std::optional<size_t>(0), 1);
    Chunk one_row = without_key.convertToBlock({0.5});
    (void)one_row;
    Chunk out = agg.convertToBlock();
    for (auto & col : q_x.quantilesForKeys(*out.columns.at(0), levels))
        out.columns.push_back(col);
    out.columns.push_back(q_y_if.quantilesForKeys(*out.columns.at(0), {0.5}, CHGPU_QUANTILE_EXACT_LOW).at(0));
    return out;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_host_only_parts_under_address_and_undefined_sanitizers(tmp_path):
    # ranks, level checks, value keys, window packing, unit arithmetic and the plan lines need no device: a stand-alone program with
    # its own main, run as a plain executable
    exe = tmp_path / "quantile_exact_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "quantile_exact_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "quantile_exact_driver OK" in r.stdout, r.stdout + r.stderr
