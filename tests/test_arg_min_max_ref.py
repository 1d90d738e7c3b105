"""The row-order restatement of argMin / argMax (tests/arg_min_max_ref.py) pinned on hand-written cases, the two enum values in the
header and in _capi, and a syntax-only compile of the shim with a two-argument AggregateDescription.  No GPU."""
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import arg_min_max_ref as R  # noqa: E402


def _one(is_min, arg, val, keys=None):
    r = R.Ref(is_min, np.asarray(arg).dtype)
    r.add_block(keys, arg, val)
    return r


def test_the_documentation_salary_table():
    # the documentation's example of argMax / argMin: user, salary
    user = np.array([0, 1, 2], dtype=np.uint8)  # director, manager, worker
    names = ["director", "manager", "worker"]
    salary = np.array([5000, 3000, 1000], dtype=np.uint32)
    assert names[int(_one(False, user, salary).result()[None])] == "director"
    assert names[int(_one(True, user, salary).result()[None])] == "worker"


def test_ties_keep_the_first_row():
    arg = np.arange(6, dtype=np.int32)
    val = np.array([3, 7, 7, 1, 1, 7], dtype=np.int16)
    assert int(_one(False, arg, val).result()[None]) == 1
    assert int(_one(True, arg, val).result()[None]) == 3
    keys = np.array([5, 5, 9, 9, 5, 9], dtype=np.uint64)
    assert {k: int(v) for k, v in _one(False, arg, val, keys).result().items()} == {5: 1, 9: 2}


def test_ties_across_blocks_keep_the_earlier_block():
    r = R.Ref(False, np.int64)
    r.add_block(None, np.array([10], dtype=np.int64), np.array([4.0]))
    r.add_block(None, np.array([11, 12], dtype=np.int64), np.array([4.0, 5.0]))
    r.add_block(None, np.array([13], dtype=np.int64), np.array([5.0]))
    assert int(r.result()[None]) == 12


def test_merge_with_equal_val_keeps_the_destination():
    a, b = _one(False, np.array([1], dtype=np.uint16), np.array([9], dtype=np.uint8)), _one(False, np.array([2], dtype=np.uint16), np.array([9], dtype=np.uint8))
    a.merge(b)
    assert int(a.result()[None]) == 1
    c = _one(False, np.array([3], dtype=np.uint16), np.array([10], dtype=np.uint8))
    a.merge(c)
    assert int(a.result()[None]) == 3
    # a later row that only equals the merged-in extremum loses to it
    a.add_block(None, np.array([4], dtype=np.uint16), np.array([10], dtype=np.uint8))
    assert int(a.result()[None]) == 3
    # argMin mirrors it
    m, n = _one(True, np.array([1], dtype=np.uint16), np.array([-5], dtype=np.int8)), _one(True, np.array([2], dtype=np.uint16), np.array([-5], dtype=np.int8))
    m.merge(n)
    assert int(m.result()[None]) == 1
    m.merge(_one(True, np.array([7], dtype=np.uint16), np.array([-6], dtype=np.int8)))
    assert int(m.result()[None]) == 7


def test_the_two_zeros_are_equal():
    arg = np.array([1, 2, 3], dtype=np.uint64)
    for dt in (np.float32, np.float64):
        assert int(_one(False, arg, np.array([-0.0, 0.0, -0.0], dtype=dt)).result()[None]) == 1
        assert int(_one(True, arg, np.array([0.0, -0.0, 0.0], dtype=dt)).result()[None]) == 1
        assert int(_one(False, arg, np.array([-1.0, -0.0, 0.0], dtype=dt)).result()[None]) == 2
    assert R.val_keys(np.array([-0.0]), False) == R.val_keys(np.array([0.0]), False)


def test_the_val_key_sorts_like_the_value():
    for vals in (np.array([-np.inf, -3.5, -0.0, 1e-300, 2.0, np.inf]), np.array([-128, -1, 0, 1, 127], dtype=np.int8),
                 np.array([0, 1, 2**63, 2**64 - 1], dtype=np.uint64), np.array([-np.inf, -1.5, 0.0, 3.25, np.inf], dtype=np.float32)):
        k = R.val_keys(vals, False)
        assert k == sorted(k) and len(set(k)) == len(k)
        km = R.val_keys(vals, True)
        assert km == sorted(km, reverse=True)
        assert all(a + b == R.M64 for a, b in zip(k, km))


def test_arg_bits_come_back_untouched():
    nan_payload = np.array([0x7FF8_0000_0000_1234, 0x8000_0000_0000_0000], dtype=np.uint64).view(np.float64)
    r = _one(False, nan_payload, np.array([2, 1], dtype=np.uint8))
    assert r.result_bytes()[None] == nan_payload[:1].tobytes()
    r = _one(True, nan_payload, np.array([2, 1], dtype=np.uint8))
    assert r.result_bytes()[None] == nan_payload[1:].tobytes()  # -0.0


def test_an_empty_state_gives_the_default_and_loses_every_merge():
    r = R.Ref(False, np.int32)
    assert r.result() == {}
    assert r.result_of(None) == 0 and r.result_of(R.State()) == 0
    full = _one(False, np.array([42], dtype=np.int32), np.array([0], dtype=np.uint64))  # the smallest key there is: still a value
    st = full.states[None].copy()
    st.merge(R.State())
    assert st.has and int(st.arg) == 42
    empty = R.State()
    empty.merge(full.states[None])
    assert empty.has and int(empty.arg) == 42


def test_find_only_rows_go_to_the_overflow_state():
    r = _one(False, np.array([1, 2], dtype=np.int64), np.array([5, 6], dtype=np.int64), keys=np.array([10, 20], dtype=np.uint32))
    ovf = R.State()
    r.add_block_find_only(np.array([10, 30, 40, 30], dtype=np.uint32), np.array([3, 4, 5, 6], dtype=np.int64), np.array([9, 7, 8, 8], dtype=np.int64), ovf)
    assert {k: int(v) for k, v in r.result().items()} == {10: 3, 20: 2}
    assert int(ovf.arg) == 5


def test_group_reference_agrees_with_the_row_loop():
    rng = np.random.Generator(np.random.PCG64(3))
    keys = rng.integers(0, 40, size=2000, dtype=np.uint64)
    val = rng.integers(-5, 5, size=2000, dtype=np.int64)
    arg = np.arange(2000, dtype=np.int64)
    mask = rng.integers(0, 2, size=2000, dtype=np.uint8)
    for is_min in (False, True):
        r = R.Ref(is_min, np.int64)
        r.add_block(keys, arg, val, mask=mask)
        assert {k: int(v) for k, v in r.result().items()} == R.group_reference(keys, arg, val, is_min, mask)


def test_enum_values_in_the_header_and_capi():
    from clickhouse_amd import _capi
    import clickhouse_amd
    assert (_capi.AGG_ARG_MIN, _capi.AGG_ARG_MAX) == (6, 7)
    assert (clickhouse_amd.AGG_ARG_MIN, clickhouse_amd.AGG_ARG_MAX) == (6, 7)
    with open(os.path.join(REPO, "include", "chgpu.h")) as f:
        text = f.read()
    assert "CHGPU_AGG_ARG_MIN = 6" in text and "CHGPU_AGG_ARG_MAX = 7" in text


def test_python_aggregator_counts_three_words_and_arg_dtype():
    from clickhouse_amd import _capi as K
    from clickhouse_amd.aggregator import Aggregator
    ag = Aggregator.__new__(Aggregator)  # (no context: only the shape helpers)
    ag.aggs = [(K.AGG_COUNT, K.U64), (K.AGG_ARG_MAX, K.F32), (K.AGG_ANY, K.I64), (K.AGG_ARG_MIN, K.I8)]
    assert ag.n_words == 1 + 3 + 2 + 3
    assert [np.dtype(d) for d in ag.result_dtypes()] == [np.dtype(x) for x in (np.uint64, np.float32, np.int64, np.int8)]


def test_shim_two_argument_description_compiles(tmp_path):
    # syntax-only: a two-argument AggregateDescription beside the one-argument initialisers existing drivers use (no GPU, no library)
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
void drive(ContextPtr ctx, Chunk chunk)
{
    std::vector<AggregateDescription> aggs{{CHGPU_AGG_COUNT, CHGPU_U64, 0}, {CHGPU_AGG_ARG_MAX, CHGPU_F64, 1, CHGPU_I64, 2}, {CHGPU_AGG_MAX, CHGPU_I64, 2}};
    static_assert(sizeof(AggregateDescription::argument2) == sizeof(size_t), "second argument position");
    if (aggs[1].stateWords() != 3 || !aggs[1].twoArguments() || aggs[2].twoArguments())
        return;
    std::vector<int> types;
    for (auto & a : aggs)
        a.appendArgumentTypes(types); // 4 slots
    auto agg = std::make_shared<GpuAggregator>(ctx, CHGPU_U32, aggs);
    agg->executeOnBlock(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0));
    Chunk out = agg->convertToBlock();
    (void)out.num_rows;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
