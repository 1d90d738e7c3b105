"""tests/window_frames_ref.py against itself and against tests/window_ref.py, without a GPU: the per-row definition and the fast form
agree on random layouts over every frame shape, both agree with window_ref wherever that serves the frame, and a few RANGE frames are
pinned by hand, the overflow cases of the contract among them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_frames_ref as F  # noqa: E402
import window_ref as R  # noqa: E402

INT_DTYPES = (np.int64, np.uint64, np.int32, np.uint32, np.int16, np.uint16, np.int8, np.uint8)
K_VALUES = (0, 1, 2, 3, 9, 2**63, 2**64 - 1)


def _values(rng, rows, dtype):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        x = rng.standard_normal(rows).astype(dt)
        special = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf], dtype=dt)
        at = rng.random(rows) < 0.3
        x[at] = rng.choice(special, size=int(at.sum()))
        return x
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=rows, dtype=dt, endpoint=True)


def _same(function, a, b):
    return (R.same_avg if function == R.AVG else R.same_bits)(a, b)


def _check_both(function, p, o, rows, frame, x, offset, default, descending):
    args = (function, [p], [o], rows, frame, None if function == R.COUNT else x)
    slow = F.window_slow(*args, offset=offset, default=default, descending=descending)
    fast = F.window_fast(*args, offset=offset, default=default, descending=descending)
    assert _same(function, slow, fast), (function, frame, descending)
    return slow


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype", INT_DTYPES, ids=[np.dtype(d).name for d in INT_DTYPES])
def test_slow_and_fast_agree_on_range_offsets(dtype, descending):
    rng = np.random.Generator(np.random.PCG64(40 + np.dtype(dtype).num))
    rows = 130
    p, _ = R.geometric_layout(rng, rows, 12.0)
    part = R.heads_fast([p], [], rows)[0]
    o = F.sorted_order(rng, part, dtype, descending, at_limits=True)
    x = _values(rng, rows, np.int32)
    xf = _values(rng, rows, np.float32)
    seen = 0
    for n, (k, m) in enumerate([(k, m) for k in K_VALUES for m in K_VALUES]):
        frames = F.range_offset_frames(k, m)
        frame = frames[n % len(frames)]
        for function in F.FRAME_FUNCTIONS:
            arg = xf if function in (R.MIN, R.MAX, R.FIRST_VALUE) else x
            _check_both(function, p, o, rows, frame, arg, n % 4, arg.dtype.type(3), descending)
            seen += 1
    assert seen == len(K_VALUES) ** 2 * len(F.FRAME_FUNCTIONS)


@pytest.mark.parametrize("dtype", [np.int64, np.float64, np.float32, np.uint8], ids=["int64", "float64", "float32", "uint8"])
def test_slow_and_fast_agree_on_two_sided_extrema(dtype):
    rng = np.random.Generator(np.random.PCG64(7))
    rows = 200
    p, o = R.geometric_layout(rng, rows, 25.0)
    x = _values(rng, rows, dtype)
    for k in (0, 1, 5, 70, 2**64 - 1):
        for m in (0, 2, 64, 2**64 - 1):
            for frame in F.two_sided_frames(k, m) + [(R.RANGE, R.CURRENT_ROW, 0, R.CURRENT_ROW, 0)]:
                for function in (R.MIN, R.MAX):
                    _check_both(function, p, o, rows, frame, x, 1, 0, False)


def test_both_agree_with_window_ref_wherever_it_serves_the_frame():
    rng = np.random.Generator(np.random.PCG64(8))
    rows = 150
    p, o = R.geometric_layout(rng, rows, 20.0)
    xi, xf = _values(rng, rows, np.int64), _values(rng, rows, np.float64)
    frames = []
    for k in (0, 1, 7, rows + 1):
        for m in (0, 2, rows + 1):
            frames += [f for f in R.frame_families(k, m) if f not in frames]
    checked = 0
    for frame in frames:
        for function in F.FRAME_FUNCTIONS:
            if function in (R.MIN, R.MAX) and not R.frame_serves_extremum(frame):
                continue
            x = None if function == R.COUNT else xi if function in (R.SUM, R.AVG, R.LAG_IN_FRAME) else xf
            default = 0 if x is None else x.dtype.type(-5)
            want = R.window_fast(function, [p], [o], rows, frame, x, offset=2, default=default)
            for ref in (F.window_slow, F.window_fast):
                assert _same(function, ref(function, [p], [o], rows, frame, x, offset=2, default=default), want), (function, frame, ref.__name__)
                checked += 1
    assert checked > 300
    for function in (R.ROW_NUMBER, R.RANK, R.DENSE_RANK):
        assert R.same_bits(F.window_fast(function, [p], [o], rows), R.window_fast(function, [p], [o], rows))
        assert R.same_bits(F.window_slow(function, [p], [o], rows), R.window_fast(function, [p], [o], rows))


def test_range_frames_pinned_by_hand():
    p = np.zeros(7, dtype=np.uint32)
    o = np.array([1, 3, 3, 4, 8, 8, 20], dtype=np.int64)
    ones = np.ones(7, dtype=np.int64)
    # 2 PRECEDING .. 1 FOLLOWING over the values: [x - 2, x + 1]
    frame = (R.RANGE, R.OFFSET_PRECEDING, 2, R.OFFSET_FOLLOWING, 1)
    assert F.window_slow(R.COUNT, [p], [o], 7, frame).tolist() == [1, 4, 4, 3, 2, 2, 1]
    assert F.window_slow(R.SUM, [p], [o], 7, frame, ones).tolist() == [1, 4, 4, 3, 2, 2, 1]
    # 5 FOLLOWING .. 12 FOLLOWING: empty where no value lies in [x + 5, x + 12]
    ahead = (R.RANGE, R.OFFSET_FOLLOWING, 5, R.OFFSET_FOLLOWING, 12)
    assert F.window_slow(R.COUNT, [p], [o], 7, ahead).tolist() == [2, 2, 2, 0, 1, 1, 0]
    assert F.window_slow(R.MAX, [p], [o], 7, ahead, o).tolist() == [8, 8, 8, 0, 20, 20, 0]
    # descending: the values negated, so the frame of x is [x - 1, x + 2]
    assert F.window_slow(R.COUNT, [p], [o[::-1].copy()], 7, frame, descending=True).tolist() == [1, 2, 2, 3, 3, 3, 3]
    # offset 0 is the peer group
    peers = (R.RANGE, R.OFFSET_PRECEDING, 0, R.OFFSET_FOLLOWING, 0)
    assert F.window_slow(R.COUNT, [p], [o], 7, peers).tolist() == [1, 2, 2, 1, 2, 2, 1]


def test_offsets_that_leave_the_type_are_exact():
    p = np.zeros(4, dtype=np.uint8)
    o = np.array([-128, -1, 0, 127], dtype=np.int8)
    # x - 200 lies below Int8's minimum for every row: every row of the partition up to the current one is >= it
    assert F.window_slow(R.COUNT, [p], [o], 4, (R.RANGE, R.OFFSET_PRECEDING, 200, R.CURRENT_ROW, 0)).tolist() == [1, 2, 3, 3]
    assert F.window_slow(R.COUNT, [p], [o], 4, (R.RANGE, R.OFFSET_PRECEDING, 255, R.CURRENT_ROW, 0)).tolist() == [1, 2, 3, 4]
    # x + 200 lies above its maximum except for the first row: no row is > it
    assert F.window_slow(R.COUNT, [p], [o], 4, (R.RANGE, R.CURRENT_ROW, 0, R.OFFSET_FOLLOWING, 200)).tolist() == [3, 3, 2, 1]
    u = np.array([0, 1, 2**64 - 1], dtype=np.uint64)
    assert F.window_slow(R.COUNT, [p[:3]], [u], 3, (R.RANGE, R.OFFSET_PRECEDING, 2**64 - 1, R.OFFSET_FOLLOWING, 2**64 - 1)).tolist() == [3, 3, 3]
    assert F.window_slow(R.COUNT, [p[:3]], [u], 3, (R.RANGE, R.OFFSET_FOLLOWING, 2**63, R.OFFSET_FOLLOWING, 2**64 - 1)).tolist() == [1, 1, 0]
    assert F.window_fast(R.COUNT, [p[:3]], [u], 3, (R.RANGE, R.OFFSET_FOLLOWING, 2**63, R.OFFSET_FOLLOWING, 2**64 - 1)).tolist() == [1, 1, 0]
