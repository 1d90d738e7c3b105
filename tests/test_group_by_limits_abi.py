"""The C ABI of max_rows_to_group_by / group_by_overflow_mode / overflow_row without a GPU: every new entry point answers a NULL handle
with BAD_ARGUMENTS and a message (the checks that need a context are in test_gpu_group_by_limits.py)."""
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


def test_overflow_modes_match_the_header(K):
    assert (K.OVERFLOW_THROW, K.OVERFLOW_BREAK, K.OVERFLOW_ANY) == (0, 1, 2)
    with open(os.path.join(REPO, "include", "chgpu.h")) as f:
        text = f.read()
    for name, v in (("THROW", 0), ("BREAK", 1), ("ANY", 2)):
        assert f"CHGPU_OVERFLOW_{name} = {v}" in text


def test_set_limits_rejects_null(K):
    _expect_bad(K, K.lib().chgpu_agg_set_limits(None, 10, K.OVERFLOW_ANY, 1))


def test_execute_on_block_rejects_null(K):
    nmk, keep = C.c_int(0), C.c_int(1)
    _expect_bad(K, K.lib().chgpu_agg_execute_on_block(None, None, None, 0, 0, None, C.byref(nmk), C.byref(keep)))


def test_merge_limited_rejects_null(K):
    nmk, keep = C.c_int(0), C.c_int(1)
    _expect_bad(K, K.lib().chgpu_agg_merge_limited(None, None, C.byref(nmk), C.byref(keep)))


def test_merge_states_limited_rejects_null(K):
    nmk, keep = C.c_int(0), C.c_int(1)
    _expect_bad(K, K.lib().chgpu_agg_merge_states_limited(None, None, None, 0, 1, C.byref(nmk), C.byref(keep)))


def test_overflow_row_rejects_null(K):
    cols = (C.c_void_p * 1)()
    has = C.c_int(7)
    _expect_bad(K, K.lib().chgpu_agg_overflow_row(None, 1, cols, C.byref(has)))


def test_python_aggregator_rejects_an_unknown_mode(K):
    from clickhouse_amd.aggregator import Aggregator
    with pytest.raises(ValueError):
        Aggregator("uint64", [], max_rows_to_group_by=1, group_by_overflow_mode="sometimes", ctx=object())


def test_shim_members_compile(tmp_path):
    # syntax-only: the shim's GROUP BY limit members as a driver uses them (no GPU, no library)
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
void drive(ContextPtr ctx, Chunk chunk)
{
    GroupByLimits lim;
    lim.max_rows_to_group_by = 10;
    lim.group_by_overflow_mode = CHGPU_OVERFLOW_ANY;
    lim.overflow_row = true;
    auto agg = std::make_shared<GpuAggregator>(ctx, CHGPU_U32, std::vector<AggregateDescription>{{CHGPU_AGG_COUNT, CHGPU_U64, 0}}, 0, lim);
    bool no_more_keys = false;
    bool keep = agg->executeOnBlock(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0), no_more_keys);
    GpuAggregator other(ctx, CHGPU_U32, {{CHGPU_AGG_COUNT, CHGPU_U64, 0}}, 0, lim);
    bool merge_no_more_keys = false;
    keep = keep && agg->mergeLimited(other, merge_no_more_keys);
    Chunk ovf = agg->convertOverflowRow();
    (void)ovf.is_overflows;
    GpuAggregatingTransform tr(agg, std::optional<size_t>(0));
    tr.consume(std::move(chunk));
    if (!tr.isConsumeFinished())
        tr.work();
}
''')
    import subprocess
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
