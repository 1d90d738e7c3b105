"""The C ABI of the -If combinator / Nullable arguments without a GPU: the enum matches the header and every new entry point answers a
NULL handle with BAD_ARGUMENTS and a message (the checks that need a context are in test_gpu_agg_conditions.py)."""
import ctypes as C
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


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


def test_condition_modes_match_the_header(K):
    assert (K.AGG_COND_NONE, K.AGG_COND_IF, K.AGG_COND_NULL) == (0, 1, 2)
    with open(os.path.join(REPO, "include", "chgpu.h")) as f:
        text = f.read()
    assert "enum { CHGPU_AGG_COND_NONE = 0, CHGPU_AGG_COND_IF = 1, CHGPU_AGG_COND_NULL = 2 };" in text


def test_new_entry_points_are_declared_and_exported(K):
    for name in ("chgpu_agg_set_conditions", "chgpu_agg_execute_on_block_conditional", "chgpu_agg_finalize_nullable"):
        assert name in K.declared_symbols() and name in K.SIGNATURES
        assert getattr(K.lib(), name)
    assert K.lib().chgpu_abi_version() == 1


def test_set_conditions_rejects_null(K):
    modes = (C.c_int * 1)(K.AGG_COND_IF)
    _expect_bad(K, K.lib().chgpu_agg_set_conditions(None, modes))


def test_execute_on_block_conditional_rejects_null(K):
    nmk, keep = C.c_int(0), C.c_int(1)
    _expect_bad(K, K.lib().chgpu_agg_execute_on_block_conditional(None, None, None, None, 0, 0, None, C.byref(nmk), C.byref(keep)))
    _expect_bad(K, K.lib().chgpu_agg_execute_on_block_conditional(None, None, None, None, 0, 0, None, None, None))


def test_finalize_nullable_rejects_null(K):
    res, maps = (C.c_void_p * 1)(), (C.c_void_p * 1)()
    n = C.c_uint64(0)
    _expect_bad(K, K.lib().chgpu_agg_finalize_nullable(None, None, res, maps, C.byref(n)))


def test_python_aggregator_rejects_an_unknown_condition(K):
    from clickhouse_amd.aggregator import Aggregator
    with pytest.raises(ValueError):
        Aggregator("uint64", [(K.AGG_SUM, "int64", "unless")], ctx=object())


def test_python_word_count_includes_the_seen_words(K):
    from clickhouse_amd.aggregator import Aggregator
    a = Aggregator.__new__(Aggregator)
    a.aggs = [(K.AGG_SUM, K.I64), (K.AGG_SUM, K.I64), (K.AGG_SUM, K.I64), (K.AGG_MIN, K.I64), (K.AGG_MAX, K.I64), (K.AGG_AVG, K.I64), (K.AGG_ANY, K.I64),
              (K.AGG_ARG_MAX, K.I64), (K.AGG_COUNT, K.U64)]
    a.cond_modes = [K.AGG_COND_NONE, K.AGG_COND_IF, K.AGG_COND_NULL, K.AGG_COND_IF, K.AGG_COND_NULL, K.AGG_COND_NULL, K.AGG_COND_IF, K.AGG_COND_NULL, K.AGG_COND_NULL]
    assert a._words_per_agg() == [1, 1, 2, 2, 2, 2, 2, 3, 1]
    assert a._reached_words() == [None, None, 3, None, 7, 9, None, 13, None]
    a._h = None


def test_shim_members_compile(tmp_path):
    # syntax-only: the shim's condition members as a driver uses them (no GPU, no library)
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
void drive(ContextPtr ctx, Chunk chunk)
{
    AggregateDescription sum_if{CHGPU_AGG_SUM, CHGPU_I64, 1};
    sum_if.condition_mode = CHGPU_AGG_COND_IF;
    sum_if.condition = 2;
    AggregateDescription min_null{CHGPU_AGG_MIN, CHGPU_I64, 1};
    min_null.condition_mode = CHGPU_AGG_COND_NULL;
    min_null.condition = 3;
    GpuAggregator agg(ctx, CHGPU_U32, {sum_if, min_null}, 0);
    size_t words = agg.stateWords() + sum_if.stateWords() + (min_null.nullableResult() ? 1 : 0);
    (void)words;
    agg.executeOnBlock(chunk.columns, 0, chunk.num_rows, std::nullopt);
    Chunk out = agg.convertToBlock();
    (void)out;
}
''')
    import subprocess
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
