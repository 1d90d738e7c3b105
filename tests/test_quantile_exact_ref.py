"""tests/quantile_exact_ref.py against a second, independent statement of the same contract: sorted() per key and the rank of each
kind written out; the pinned ranks; NaN and the empty state; the constants it mirrors from clickhouse_amd/csrc/quantile_host.h."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantile_exact_ref as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _values(rng, dtype, n, nan_share=0.1):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        v = rng.standard_normal(n).astype(dtype) * dtype.type(1000)
        pool = np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(dtype).tiny / 4, np.finfo(dtype).max, np.finfo(dtype).min], dtype=dtype)
        pick = rng.random(n) < 0.2
        v[pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
        v[rng.random(n) < nan_share] = np.nan
        return v
    info = np.iinfo(dtype)
    v = rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)
    if n >= 2:
        v[0], v[1] = info.min, info.max
    return v


def _second_statement(keys, values, levels, kind):
    """per key: sorted() of the values that are not NaN, then the rank of the kind spelled out"""
    per_key = {}
    for k, v in zip(keys, values.tolist()):
        if isinstance(v, float) and math.isnan(v):
            continue
        per_key.setdefault(k, []).append(v)
    out = {}
    for k, vals in per_key.items():
        vals = sorted(vals)
        n = len(vals)
        row = []
        for l in levels:
            if kind == "low" and l == 0.5:
                r = (n - 1) // 2
            elif kind == "high" and l == 0.5:
                r = n // 2
            elif l >= 1:
                r = n - 1
            else:
                r = math.floor(l * n)   # float * int: the same IEEE product
            row.append(vals[r])
        out[k] = row
    return out


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_reference_equals_the_second_statement(dtype):
    rng = _rng(7 + np.dtype(dtype).num)
    levels = [0.0, 0.07, 0.25, 0.29, 0.5, 0.57, 0.9, 0.99, 1.0]
    for n in list(range(0, 12)) + [63, 64, 65, 100, 299, 300]:
        values = _values(rng, dtype, n)
        keys = rng.integers(0, 5, size=n).astype(np.uint16)
        for kind in R.KINDS:
            ref = R.QuantileExactRef(np.uint16, dtype).add(keys, values)
            got = ref.finalize(levels, kind)
            want = _second_statement(keys.tolist(), values, levels, kind)
            assert sorted(got) == sorted(want)
            for k in want:
                assert R.same(np.array(got[k], dtype=dtype), np.array(want[k], dtype=dtype)), (n, kind, k)
            nokey = R.QuantileExactRef(None, dtype).add(None, values).finalize(levels, kind)[None]
            want0 = _second_statement([0] * n, values, levels, kind).get(0)
            if want0 is None:
                assert R.same(np.array(nokey, dtype=dtype), np.array([R.empty_value(dtype)] * len(levels), dtype=dtype))
            else:
                assert R.same(np.array(nokey, dtype=dtype), np.array(want0, dtype=dtype))


def test_pinned_ranks():
    assert R.rank("exact", 0.29, 100) == 28     # 0.29 * 100 = 28.999999999999996
    assert R.rank("exact", 0.57, 100) == 56
    assert R.rank("exact", 0.07, 100) == 7
    for n in (1, 2, 3, 100, 2049):
        assert R.rank("exact", 1.0, n) == n - 1
        assert R.rank("exact", 0.0, n) == 0
    ref = R.QuantileExactRef(None, np.int32).add(None, np.arange(100, dtype=np.int32)[::-1].copy())
    assert [int(x) for x in ref.finalize([0.29, 0.57, 1.0, 0.0])[None]] == [28, 56, 99, 0]


def test_low_and_high_differ_from_exact_at_one_half_only():
    for n, low, high in ((1, 0, 0), (2, 0, 1), (3, 1, 1), (4, 1, 2), (5, 2, 2), (100, 49, 50), (101, 50, 50)):
        assert R.rank("low", 0.5, n) == low and R.rank("high", 0.5, n) == high
        assert R.rank("exact", 0.5, n) == n // 2
        for kind in ("low", "high"):
            assert R.rank(kind, 0.25, n) == R.rank("exact", 0.25, n)
            assert R.rank(kind, 1.0, n) == n - 1 and R.rank(kind, 0.0, n) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_nan_never_enters(dtype):
    values = np.array([np.nan, 3.0, np.nan, 1.0, 2.0], dtype=dtype)
    ref = R.QuantileExactRef(None, dtype).add(None, values)
    assert ref.nan == 2 and len(ref) == 3
    assert [float(x) for x in ref.finalize([0.0, 0.5, 1.0])[None]] == [1.0, 2.0, 3.0]
    all_nan = R.QuantileExactRef(np.uint8, dtype).add(np.zeros(4, dtype=np.uint8), np.full(4, np.nan, dtype=dtype))
    assert all_nan.nan == 4 and len(all_nan) == 0 and all_nan.finalize([0.5]) == {}
    assert np.isnan(all_nan.for_keys(np.zeros(2, dtype=np.uint8), [0.5])[0]).all()
    assert np.isnan(R.QuantileExactRef(None, dtype).finalize([0.5])[None][0])


def test_empty_state_value():
    for dtype in R.DTYPES:
        e = R.empty_value(dtype)
        assert e.dtype == np.dtype(dtype)
        assert np.isnan(e) if np.dtype(dtype).kind == "f" else e == 0
        assert R.same(np.array(R.QuantileExactRef(None, dtype).finalize([0.1, 0.9])[None], dtype=dtype), np.array([e, e], dtype=dtype))


def test_filter_rows_merge_and_pairs():
    keys = np.array([1, 1, 2, 2, 2, 3], dtype=np.int8)
    values = np.array([5, 4, 3, 2, 1, 0], dtype=np.int64)
    a = R.QuantileExactRef(np.int8, np.int64).add(keys, values, 1, 5, filter=np.array([1, 1, 0, 1, 1, 1], dtype=np.uint8))
    assert a.pairs() == [(1, 4), (2, 1), (2, 2)]
    b = R.QuantileExactRef(np.int8, np.int64).add(keys, values)
    a.merge(b)
    assert len(a) == 9 and a.finalize([0.5])[2][0] == 2 and a.classes() == (3, 0, 0)
    assert [int(x) for x in a.for_keys(np.array([3, 9, 1], dtype=np.int8), [1.0])[0]] == [0, 0, 5]
    # a signed key is its bits zero-extended
    neg = R.QuantileExactRef(np.int8, np.int64).add(np.array([-1], dtype=np.int8), np.array([7], dtype=np.int64))
    assert list(neg.finalize([0.5])) == [255]


def test_same_compares_zeros_numerically_and_everything_else_as_bits():
    assert R.same(np.array([0.0, 1.0]), np.array([-0.0, 1.0]))
    assert not R.same(np.array([1.0]), np.array([1.0000000000000002]))
    assert R.same(np.array([np.nan]), np.array([np.nan])) and not R.same(np.array([np.nan]), np.array([0.0]))
    assert not R.same(np.array([1], dtype=np.int32), np.array([1], dtype=np.int64))


def test_classes_count_segments_and_units():
    n_large = R.QT_CHUNK + 1
    keys = np.concatenate([np.zeros(R.QT_SMALL_MAX, dtype=np.uint32), np.ones(R.QT_SMALL_MAX + 1, dtype=np.uint32), np.full(n_large, 2, dtype=np.uint32)])
    ref = R.QuantileExactRef(np.uint32, np.uint8).add(keys, np.zeros(len(keys), dtype=np.uint8))
    assert ref.classes() == (1, 2, 1 + 2)


def test_constants_mirror_the_header():
    text = open(os.path.join(REPO, "clickhouse_amd", "csrc", "quantile_host.h")).read()
    for name in ("QT_SMALL_MAX", "QT_CHUNK"):
        m = re.search(r"static constexpr uint64_t %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == getattr(R, name), name
    m = re.search(r"#define CHGPU_QUANTILE_MAX_LEVELS (\d+)", open(os.path.join(REPO, "include", "chgpu.h")).read())
    assert m and int(m.group(1)) == R.MAX_LEVELS
