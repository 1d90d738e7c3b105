"""tests/agg_conditions_ref.py (the yardstick of tests/test_gpu_agg_conditions.py) on hand-written rows: no device involved."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import agg_conditions_ref as R  # noqa: E402

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def _cols(ref, order):
    return ref.columns(order)


def test_a_group_exists_whatever_the_conditions_say():
    ref = R.Ref([(R.COUNT, None, "if"), (R.SUM, np.int64, "if")])
    ref.add_block([5, 0, 5, 9], [None, np.array([10, 20, 30, 40])], conds=[[1, 0, 2, 0], [0, 0, 255, 0]])
    assert list(ref.groups) == [5, 0, 9]
    vals, nulls = _cols(ref, [5, 0, 9])
    assert vals[0].tolist() == [2, 0, 0] and vals[0].dtype == np.uint64   # any non-zero byte counts
    assert vals[1].tolist() == [30, 0, 0] and vals[1].dtype == np.int64
    assert nulls == [None, None]


def test_where_removes_the_row_and_the_group():
    ref = R.Ref([(R.COUNT, None, "if")])
    ref.add_block([1, 2, 3], [None], conds=[[1, 1, 1]], where=[1, 0, 1])
    assert list(ref.groups) == [1, 3]


def test_if_defaults_of_an_empty_state():
    aggs = [(R.COUNT, None, "if"), (R.SUM, np.float64, "if"), (R.AVG, np.int32, "if"), (R.MIN, np.int64, "if"), (R.MAX, np.int64, "if"),
            (R.ANY, np.uint32, "if"), (R.ARG_MAX, (np.int8, np.int64), "if")]
    ref = R.Ref(aggs)
    z = [0]
    ref.add_block([7], [None, np.array([np.nan]), np.array([3], dtype=np.int32), np.array([I64_MIN]), np.array([I64_MAX]),
                        np.array([9], dtype=np.uint32), (np.array([4], dtype=np.int8), np.array([1]))], conds=[z] * 7)
    vals, nulls = _cols(ref, [7])
    assert vals[0][0] == 0
    assert vals[1].tobytes() == np.float64(0.0).tobytes()   # +0.0: the masked-out NaN left no trace
    assert math.isnan(vals[2][0])
    assert [int(vals[j][0]) for j in (3, 4, 5, 6)] == [0, 0, 0, 0]
    assert [v.dtype for v in vals] == [np.uint64, np.float64, np.float64, np.int64, np.int64, np.uint32, np.int8]
    assert nulls == [None] * 7


def test_null_mode_flags_and_nested_defaults():
    aggs = [(R.COUNT, None, "null"), (R.SUM, np.uint32, "null"), (R.AVG, np.float64, "null"), (R.MIN, np.int64, "null"), (R.ANY, np.int8, "null")]
    ref = R.Ref(aggs)
    nm = [1, 0, 1]   # key 1: both rows NULL; key 2: its row is not
    ref.add_block([1, 2, 1], [None, np.array([5, 6, 7], dtype=np.uint32), np.array([1.5, 2.5, 3.5]), np.array([I64_MIN, I64_MIN, 3]),
                              np.array([-1, -2, -3], dtype=np.int8)], conds=[nm] * 5)
    vals, nulls = _cols(ref, [1, 2])
    assert vals[0].tolist() == [0, 1] and nulls[0] is None   # count stays UInt64 without a map
    assert vals[1].tolist() == [0, 6] and nulls[1].tolist() == [1, 0]
    assert vals[2].tolist() == [0.0, 2.5] and nulls[2].tolist() == [1, 0]   # avg: 0.0, not NaN
    assert vals[3].tolist() == [0, I64_MIN] and nulls[3].tolist() == [1, 0]
    assert vals[4].tolist() == [0, -2] and nulls[4].tolist() == [1, 0]


def test_extremes_are_values_not_identities():
    ref = R.Ref([(R.MIN, np.int64, "if"), (R.MAX, np.int64, "if")])
    ref.add_block([1, 1, 2], [np.array([I64_MAX, 5, 5]), np.array([I64_MIN, 5, 5])], conds=[[1, 0, 0], [1, 0, 0]])
    vals, _ = _cols(ref, [1, 2])
    assert vals[0].tolist() == [I64_MAX, 0] and vals[1].tolist() == [I64_MIN, 0]


def test_first_row_rules_skip_masked_out_rows():
    ref = R.Ref([(R.ANY, np.int64, "if"), (R.ARG_MAX, (np.int64, np.int64), "if"), (R.ARG_MIN, (np.int64, np.int64), "null")])
    arg = np.array([100, 101, 102, 103, 104])
    val = np.array([9, 5, 7, 7, 1])
    c = [0, 1, 1, 1, 0]          # the best val (row 0) and the smallest (row 4) are masked out
    nm = [1, 0, 0, 0, 1]
    ref.add_block([3] * 5, [arg, (arg, val), (arg, val)], conds=[c, c, nm])
    vals, nulls = _cols(ref, [3])
    assert vals[0].tolist() == [101]       # the first row that reaches it
    assert vals[1].tolist() == [102]       # the first of the two 7s
    assert vals[2].tolist() == [101] and nulls[2].tolist() == [0]


def test_sums_wrap_and_float_sums_are_fsum():
    ref = R.Ref([(R.SUM, np.uint64, "if"), (R.SUM, np.int8, "if"), (R.SUM, np.float64, "if"), (R.AVG, np.int64, "if")])
    u = np.array([(1 << 64) - 1, 2, 7], dtype=np.uint64)
    i8 = np.array([-128, -128, 100], dtype=np.int8)
    f = np.array([1e16, 1.0, -1e16])
    i = np.array([-3, -4, 1000])
    ref.add_block([1, 1, 1], [u, i8, f, i], conds=[[1, 1, 0]] * 4)
    vals, _ = _cols(ref, [1])
    assert int(vals[0][0]) == 1 and int(vals[1][0]) == -256 and vals[1].dtype == np.int64
    assert vals[2][0] == math.fsum([1e16, 1.0]) and vals[3][0] == -3.5


def test_blocks_views_and_merges_agree():
    aggs = [(R.SUM, np.int64, "if"), (R.MIN, np.int64, "null"), (R.ANY, np.int64, "if"), (R.COUNT, None, None)]
    k = np.array([1, 2, 1, 3, 2, 1])
    x = np.array([10, 20, 30, 40, 50, 60])
    c = np.array([0, 1, 1, 0, 0, 1], dtype=np.uint8)
    whole = R.Ref(aggs)
    whole.add_block(k, [x, x, x, None], conds=[c, c, c, None])
    parts = R.Ref(aggs)
    parts.add_block(k, [x, x, x, None], conds=[c, c, c, None], row_end=2)
    other = R.Ref(aggs)
    other.add_block(k, [x, x, x, None], conds=[c, c, c, None], row_begin=2)
    parts.merge(other)
    assert list(parts.groups) == [1, 2, 3]   # key 3 exists in the source alone, reached by no function but count
    for a, b in zip(_cols(whole, [1, 2, 3])[0] + _cols(whole, [1, 2, 3])[1][1:2], _cols(parts, [1, 2, 3])[0] + _cols(parts, [1, 2, 3])[1][1:2]):
        assert a.tobytes() == b.tobytes()
    assert _cols(whole, [1, 2, 3])[0][0].tolist() == [90, 20, 0]
    assert _cols(whole, [1, 2, 3])[0][1].tolist() == [10, 50, 40] and _cols(whole, [1, 2, 3])[1][1].tolist() == [0, 0, 0]
    assert _cols(whole, [1, 2, 3])[0][2].tolist() == [30, 20, 0]


def test_find_only_rows_reach_the_overflow_row_under_their_conditions():
    aggs = [(R.COUNT, None, "if"), (R.MIN, np.int64, "if"), (R.SUM, np.int64, "null")]
    ref = R.Ref(aggs)
    ref.add_block([1], [None, np.array([5]), np.array([5])], conds=[[1], [1], [0]], overflow_row=True)
    ref.add_block([1, 8, 9], [None, np.array([1, 2, 3]), np.array([1, 2, 3])], conds=[[1, 0, 1], [0, 0, 0], [0, 1, 1]], find_only=True, overflow_row=True)
    assert list(ref.groups) == [1]
    vals, nulls = ref.overflow_columns()
    assert vals[0].tolist() == [1] and vals[1].tolist() == [0] and vals[2].tolist() == [0] and nulls[2].tolist() == [1]


def test_without_key_one_group_per_function_emptiness():
    ref = R.Ref([(R.MAX, np.int64, "if"), (R.MAX, np.int64, "if"), (R.COUNT, None, None)])
    x = np.array([4, -7])
    ref.add_block(None, [x, x, None], conds=[[0, 0], [0, 0], None])
    ref.add_block(None, [x, x, None], conds=[[0, 1], [0, 0], None])
    vals, _ = ref.columns([None])
    assert vals[0].tolist() == [-7] and vals[1].tolist() == [0] and vals[2].tolist() == [4]


def test_the_vectorised_form_equals_the_row_order_form():
    rng = np.random.Generator(np.random.PCG64(3))
    n = 3000
    k = rng.integers(0, 40, size=n).astype(np.uint32)
    a = rng.integers(-(1 << 62), 1 << 62, size=n)
    b = rng.integers(0, 1 << 32, size=n).astype(np.uint32)
    c1 = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=n)
    c2 = (rng.random(n) < 0.1).astype(np.uint8)
    w = (rng.random(n) < 0.7).astype(np.uint8)
    aggs = [(R.SUM, np.int64, None), (R.SUM, np.int64, "if"), (R.SUM, np.uint32, "null"), (R.COUNT, None, "if"), (R.AVG, np.uint32, "if"), (R.AVG, np.int64, "null")]
    args, conds = [a, a, b, None, b, a], [None, c1, c2, c2, c2, c1]
    ref = R.Ref(aggs)
    ref.add_block(k, args, conds=conds, where=w)
    gk, vals, nulls = R.additive_reference(k, args, conds, aggs, where=w)
    assert sorted(ref.groups) == gk.tolist()
    rv, rn = ref.columns(gk)
    for j in range(len(aggs)):
        assert np.array_equal(rv[j], vals[j], equal_nan=True), j
        assert (rn[j] is None and nulls[j] is None) or np.array_equal(rn[j], nulls[j]), j
