"""The window reference (tests/window_ref.py) without a GPU: the per-row form is pinned with columns written out by hand over a table of
three partitions with ties in the order key, and the vectorised form is held against the per-row form on random inputs, every function
over every served frame kind with the offsets 0, 1, one longer than any partition and 2^64 - 1."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_ref as R  # noqa: E402

NAN = float("nan")

# row          0   1   2   3   4   5   6   7   8   9
P = np.array([1,  1,  1,  1,  2,  2,  2,  3,  3,  3], dtype=np.uint32)
O = np.array([1,  1,  2,  3,  5,  5,  5,  1,  2,  2], dtype=np.int64)
X = np.array([5, -2,  7,  3,  4,  4, -9, 10, -1,  6], dtype=np.int32)


def slow(function, frame=None, x=None, **kw):
    return R.window_slow(function, [P], [O], len(P), frame, x, **kw)


def rows_frame(b, bo, e, eo):
    return (R.ROWS, b, bo, e, eo)


def test_ranks_by_hand():
    assert slow(R.ROW_NUMBER).tolist() == [1, 2, 3, 4, 1, 2, 3, 1, 2, 3]
    assert slow(R.RANK).tolist() == [1, 1, 3, 4, 1, 1, 1, 1, 2, 2]
    assert slow(R.DENSE_RANK).tolist() == [1, 1, 2, 3, 1, 1, 1, 1, 2, 2]
    assert slow(R.RANK).dtype == np.uint64


def test_count_by_hand():
    assert slow(R.COUNT).tolist() == [2, 2, 3, 4, 3, 3, 3, 1, 3, 3]                                    # default: through the last peer
    assert slow(R.COUNT, rows_frame(R.OFFSET_FOLLOWING, 1, R.UNBOUNDED_FOLLOWING, 0)).tolist() == [3, 2, 1, 0, 2, 1, 0, 2, 1, 0]
    assert slow(R.COUNT, (R.RANGE, R.CURRENT_ROW, 0, R.UNBOUNDED_FOLLOWING, 0)).tolist() == [4, 4, 2, 1, 3, 3, 3, 3, 2, 2]
    assert slow(R.COUNT, (R.RANGE, R.CURRENT_ROW, 0, R.CURRENT_ROW, 0)).tolist() == [2, 2, 1, 1, 3, 3, 3, 1, 2, 2]


def test_sum_and_avg_by_hand():
    assert slow(R.SUM, None, X).tolist() == [3, 3, 10, 13, -1, -1, -1, 10, 15, 15]
    assert slow(R.SUM, rows_frame(R.UNBOUNDED_PRECEDING, 0, R.CURRENT_ROW, 0), X).tolist() == [5, 3, 10, 13, 4, 8, -1, 10, 9, 15]
    assert slow(R.SUM, rows_frame(R.OFFSET_PRECEDING, 1, R.OFFSET_FOLLOWING, 1), X).tolist() == [3, 10, 8, 10, 8, -1, -5, 9, 15, 5]
    assert slow(R.SUM, None, X).dtype == np.int64 and slow(R.SUM, None, X.astype(np.uint16)).dtype == np.uint64
    got = slow(R.AVG, rows_frame(R.OFFSET_PRECEDING, 2, R.OFFSET_PRECEDING, 1), X)
    want = [NAN, 5.0, 1.5, 2.5, NAN, 4.0, 4.0, NAN, 10.0, 4.5]
    assert got.dtype == np.float64 and np.array_equal(got, np.array(want), equal_nan=True)


def test_sum_wraps_around():
    big = np.array([2**63 - 1, 1, 2**63 - 1], dtype=np.int64)
    one = np.zeros(3, dtype=np.uint8)
    frame = rows_frame(R.UNBOUNDED_PRECEDING, 0, R.CURRENT_ROW, 0)
    assert R.window_slow(R.SUM, [one], [], 3, frame, big).tolist() == [2**63 - 1, -2**63, -1]
    ubig = np.array([2**64 - 1, 2, 2**64 - 1], dtype=np.uint64)
    assert R.window_slow(R.SUM, [one], [], 3, frame, ubig).tolist() == [2**64 - 1, 1, 0]


def test_min_max_first_last_by_hand():
    whole = rows_frame(R.UNBOUNDED_PRECEDING, 0, R.UNBOUNDED_FOLLOWING, 0)
    assert slow(R.MAX, whole, X).tolist() == [7, 7, 7, 7, 4, 4, 4, 10, 10, 10]
    assert slow(R.MAX, None, X).tolist() == [5, 5, 7, 7, 4, 4, 4, 10, 10, 10]
    assert slow(R.MIN, rows_frame(R.CURRENT_ROW, 0, R.UNBOUNDED_FOLLOWING, 0), X).tolist() == [-2, -2, 3, 3, -9, -9, -9, -1, -1, 6]
    assert slow(R.FIRST_VALUE, rows_frame(R.OFFSET_FOLLOWING, 1, R.OFFSET_FOLLOWING, 2), X).tolist() == [-2, 7, 3, 0, 4, -9, 0, -1, 6, 0]
    assert slow(R.LAST_VALUE, (R.RANGE, R.CURRENT_ROW, 0, R.CURRENT_ROW, 0), X).tolist() == [-2, -2, 7, 3, -9, -9, -9, 10, 6, 6]
    assert slow(R.MAX, whole, X).dtype == np.int32


def test_lag_and_lead_by_hand():
    whole = rows_frame(R.UNBOUNDED_PRECEDING, 0, R.UNBOUNDED_FOLLOWING, 0)
    assert slow(R.LAG_IN_FRAME, whole, X, offset=1, default=np.int32(-7)).tolist() == [-7, 5, -2, 7, -7, 4, 4, -7, 10, -1]
    assert slow(R.LEAD_IN_FRAME, None, X, offset=2, default=np.int32(99)).tolist() == [99, 99, 99, 99, -9, 99, 99, 99, 99, 99]
    assert slow(R.LAG_IN_FRAME, whole, X, offset=0, default=np.int32(1)).tolist() == X.tolist()
    assert slow(R.LEAD_IN_FRAME, whole, X, offset=2**64 - 1, default=np.int32(1)).tolist() == [1] * 10


def test_float_order_and_float_key_equality_by_hand():
    one = np.zeros(4, dtype=np.uint8)
    whole = rows_frame(R.UNBOUNDED_PRECEDING, 0, R.UNBOUNDED_FOLLOWING, 0)
    x = np.array([0.0, -0.0, NAN, -np.inf], dtype=np.float64)
    assert np.isnan(R.window_slow(R.MAX, [one], [], 4, whole, x)).all()                                # +NaN stands above +inf
    assert R.window_slow(R.MIN, [one], [], 4, whole, x).tolist() == [-np.inf] * 4
    z = np.array([0.0, -0.0, -0.0, 0.0], dtype=np.float32)
    assert R.window_slow(R.MAX, [one], [], 4, whole, z).view(np.uint32).tolist() == [0] * 4            # +0.0 above -0.0, bits kept
    assert R.window_slow(R.MIN, [one], [], 4, whole, z).view(np.uint32).tolist() == [0x80000000] * 4
    o = np.array([0.0, -0.0, NAN, NAN, 1.0], dtype=np.float64)                                         # -0.0 equals +0.0, NaN equals NaN
    assert R.window_slow(R.RANK, [], [o], 5).tolist() == [1, 1, 3, 3, 5]
    assert R.window_slow(R.ROW_NUMBER, [o], [], 5).tolist() == [1, 2, 1, 2, 1]


def test_frame_validity_table():
    kinds = range(5)
    illegal = {(b, e) for b, e in itertools.product(kinds, kinds)
               if b == R.UNBOUNDED_FOLLOWING or e == R.UNBOUNDED_PRECEDING or (b == R.CURRENT_ROW and e == R.OFFSET_PRECEDING)
               or (b == R.OFFSET_FOLLOWING and e in (R.CURRENT_ROW, R.OFFSET_PRECEDING))}
    assert len(illegal) == 12
    for b, e in itertools.product(kinds, kinds):
        assert R.frame_is_legal((R.ROWS, b, 1, e, 1)) == ((b, e) not in illegal)
    assert not R.frame_is_legal(rows_frame(R.OFFSET_PRECEDING, 1, R.OFFSET_PRECEDING, 2))
    assert not R.frame_is_legal(rows_frame(R.OFFSET_FOLLOWING, 2, R.OFFSET_FOLLOWING, 1))
    assert R.frame_is_legal((R.RANGE, R.OFFSET_PRECEDING, 1, R.CURRENT_ROW, 0)) and not R.frame_is_served((R.RANGE, R.OFFSET_PRECEDING, 1, R.CURRENT_ROW, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# vectorised against per-row
# ---------------------------------------------------------------------------------------------------------------------------------
ROWS_N = 300
OFFSETS = (0, 1, ROWS_N + 1, 2**64 - 1)


def all_served_frames():
    out = [None]
    for t, b, e in itertools.product((R.ROWS, R.RANGE), range(5), range(5)):
        for bo, eo in itertools.product(OFFSETS, OFFSETS):
            f = (t, b, bo if b in (R.OFFSET_PRECEDING, R.OFFSET_FOLLOWING) else 0, e, eo if e in (R.OFFSET_PRECEDING, R.OFFSET_FOLLOWING) else 0)
            if R.frame_is_served(f) and f not in out:
                out.append(f)
    return out


@pytest.fixture(scope="module")
def table():
    rng = np.random.Generator(np.random.PCG64(20))
    p, o = R.geometric_layout(rng, ROWS_N, 9.0)
    xi = rng.integers(-2**63, 2**63 - 1, size=ROWS_N, dtype=np.int64)
    xu = rng.integers(0, 256, size=ROWS_N).astype(np.uint8)
    xf = rng.standard_normal(ROWS_N).astype(np.float32)
    xf[rng.integers(0, ROWS_N, 12)] = [NAN, -NAN, 0.0, -0.0, np.inf, -np.inf] * 2
    return p, o, {"i64": xi, "u8": xu, "f32": xf}


def test_the_frame_list_covers_every_kind():
    frames = all_served_frames()
    assert {(f[0], f[1], f[3]) for f in frames if f is not None} >= {(R.ROWS, b, e) for b in range(4) for e in range(1, 5)
                                                                      if R.frame_is_legal((R.ROWS, b, 1, e, 1))}
    assert (R.RANGE, R.CURRENT_ROW, 0, R.CURRENT_ROW, 0) in frames and len(frames) > 60


@pytest.mark.parametrize("function", range(12))
def test_vectorised_equals_per_row(table, function):
    p, o, xs = table
    if function in (R.ROW_NUMBER, R.RANK, R.DENSE_RANK):
        assert R.same_bits(R.window_fast(function, [p], [o], ROWS_N), R.window_slow(function, [p], [o], ROWS_N))
        assert R.same_bits(R.window_fast(function, [], [], ROWS_N), R.window_slow(function, [], [], ROWS_N))
        return
    names = [None] if function == R.COUNT else ["i64", "u8"] if function in (R.SUM, R.AVG) else ["i64", "u8", "f32"]
    for frame in all_served_frames():
        if function in (R.MIN, R.MAX) and not R.frame_serves_extremum(frame):
            continue
        for name in names:
            x = None if name is None else xs[name]
            offsets = OFFSETS if function in (R.LAG_IN_FRAME, R.LEAD_IN_FRAME) else (1,)
            for off in offsets:
                default = 0 if x is None else x.dtype.type(3)
                fast = R.window_fast(function, [p], [o], ROWS_N, frame, x, offset=off, default=default)
                slow_ = R.window_slow(function, [p], [o], ROWS_N, frame, x, offset=off, default=default)
                same = R.same_avg if function == R.AVG else R.same_bits
                assert same(fast, slow_), (function, frame, name, off)


@pytest.mark.parametrize("rows", [0, 1, 2])
def test_vectorised_equals_per_row_at_tiny_sizes(rows):
    p = np.arange(rows, dtype=np.uint32) // 2
    x = np.arange(rows, dtype=np.int16) - 1
    for function in range(12):
        arg = None if function in R.FUNCTIONS_WITHOUT_ARG else x
        fast = R.window_fast(function, [p], [], rows, None, arg, offset=1, default=np.int16(5))
        slow_ = R.window_slow(function, [p], [], rows, None, arg, offset=1, default=np.int16(5))
        assert (R.same_avg if function == R.AVG else R.same_bits)(fast, slow_), function
