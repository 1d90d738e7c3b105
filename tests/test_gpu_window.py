"""The window operator on the device against tests/window_ref.py, bit for bit (a NaN cell of an avg column is compared as NaN).

T is the scan tile and G the tile partials one pass of the one-workgroup kernel covers; the shapes are the smallest at which each
mechanism can break: sizes around the wave and the tile, heads exactly at tile edges, a partition / a peer group whose carry crosses a
tile without a head, a last partition of one row, and T * G + T + 5 rows so that the one-workgroup pass loops twice.  Inputs of up to 65
rows are checked against the per-row reference, larger ones against the vectorised one (test_window_ref.py holds the two together)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
WHOLE = (R.ROWS, R.UNBOUNDED_PRECEDING, 0, R.UNBOUNDED_FOLLOWING, 0)
RUNNING = (R.ROWS, R.UNBOUNDED_PRECEDING, 0, R.CURRENT_ROW, 0)
AHEAD = (R.ROWS, R.CURRENT_ROW, 0, R.UNBOUNDED_FOLLOWING, 0)
AROUND = (R.ROWS, R.OFFSET_PRECEDING, 3, R.OFFSET_FOLLOWING, 1)
PEERS = (R.RANGE, R.CURRENT_ROW, 0, R.CURRENT_ROW, 0)
ALL_DTYPES = (np.int64, np.uint32, np.uint64, np.float64, np.uint8, np.int32, np.uint16, np.int16, np.int8, np.float32)


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    return ch.Context(0)


@pytest.fixture(scope="module")
def T(ch):
    from clickhouse_amd import window
    assert [getattr(ch._capi, n) for n in ("WIN_ROW_NUMBER", "WIN_COUNT", "WIN_SUM", "WIN_MIN", "WIN_LEAD_IN_FRAME")] == [R.ROW_NUMBER, R.COUNT, R.SUM, R.MIN,
                                                                                                                        R.LEAD_IN_FRAME]
    return window.TILE


def to_frame(ch, f):
    if f is None:
        return None

    def bound(kind, off):
        if kind in (R.UNBOUNDED_PRECEDING, R.UNBOUNDED_FOLLOWING):
            return ch.UNBOUNDED
        return ch.CURRENT_ROW if kind == R.CURRENT_ROW else ch.preceding(off) if kind == R.OFFSET_PRECEDING else ch.following(off)
    return ch.Frame(f[0], bound(f[1], f[2]), bound(f[3], f[4]))


class Case:
    """one window over host columns, the device handle beside them"""

    def __init__(self, ch, ctx, part_cols, order_cols, rows):
        self.ch, self.ctx, self.p, self.o, self.rows = ch, ctx, list(part_cols), list(order_cols), rows
        self.win = ch.Window(self.p, self.o, ctx=ctx, rows=rows)
        self.slow = rows <= 65
        self._dev = {}

    def check(self, function, frame=None, x=None, offset=1, default=0):
        col = None
        if x is not None:
            col = self._dev.get(id(x))
            if col is None:
                col = self._dev[id(x)] = self.ctx.upload(x)
        if x is not None:
            default = x.dtype.type(default)
        got = self.win.evaluate_column(function, to_frame(self.ch, frame), col, offset, default).numpy()
        ref = R.window_slow if self.slow else R.window_fast
        want = ref(function, self.p, self.o, self.rows, frame, x, offset=offset, default=default)
        same = R.same_avg if function == R.AVG else R.same_bits
        assert got.dtype == want.dtype and same(got, want), (function, frame, None if x is None else x.dtype, offset, _first_difference(got, want))

    def check_every_function(self, x, frames):
        for f in (R.ROW_NUMBER, R.RANK, R.DENSE_RANK):
            self.check(f)
        for frame in frames:
            self.check(R.COUNT, frame)
            if x.dtype.kind != "f":
                self.check(R.SUM, frame, x)
                self.check(R.AVG, frame, x)
            if R.frame_serves_extremum(frame):
                self.check(R.MIN, frame, x)
                self.check(R.MAX, frame, x)
            self.check(R.FIRST_VALUE, frame, x)
            self.check(R.LAST_VALUE, frame, x)
            self.check(R.LAG_IN_FRAME, frame, x, 1, 3)
            self.check(R.LEAD_IN_FRAME, frame, x, 2, 4)


def _first_difference(got, want):
    a, b = got.view(f"u{got.dtype.itemsize}"), want.view(f"u{want.dtype.itemsize}")
    if a.shape != b.shape:
        return (a.shape, b.shape)
    d = np.flatnonzero(a != b)
    return None if not len(d) else (int(d[0]), got[d[0]], want[d[0]], len(d))


def values(rng, rows, dtype=np.int64):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return rng.standard_normal(rows).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=rows, dtype=dt, endpoint=True)


def sizes(T):
    return [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# sizes, tile edges, carries
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_partition", [False, True], ids=["one-partition", "row-per-partition"])
@pytest.mark.parametrize("size_index", range(10))
def test_sizes_around_the_wave_and_the_tile(ch, ctx, T, size_index, own_partition):
    rows = sizes(T)[size_index]
    rng = np.random.Generator(np.random.PCG64(100 + size_index))
    p = np.arange(rows, dtype=np.uint32) if own_partition else np.full(rows, 7, dtype=np.uint32)
    o = (np.arange(rows, dtype=np.int64) // 3) if not own_partition else np.zeros(rows, dtype=np.int64)
    case = Case(ch, ctx, [p], [o], rows)
    case.check_every_function(values(rng, rows, np.int32), [None, WHOLE, AROUND, AHEAD, PEERS])
    parts, peers = R.heads_fast([p], [o], rows)
    assert case.win.counts() == (rows, int(parts.sum()), int(peers.sum()))


def test_partition_heads_exactly_at_tile_edges(ch, ctx, T):
    rows = 2 * T + 40
    rng = np.random.Generator(np.random.PCG64(1))
    p = (np.arange(rows) // T).astype(np.uint16)                     # heads at rows T and 2T
    o = np.zeros(rows, dtype=np.int8)
    o[T - 1:] = 1                                                    # a peer head on the last row of tile 0 ...
    o[2 * T + 1:] = 2                                                # ... and on the second row of tile 2
    Case(ch, ctx, [p], [o], rows).check_every_function(values(rng, rows, np.int64), [None, WHOLE, RUNNING, AROUND, AHEAD, PEERS])


def test_a_partition_crosses_a_tile_without_a_head_and_the_last_partition_is_one_row(ch, ctx, T):
    rows = 4 * T + 1
    rng = np.random.Generator(np.random.PCG64(2))
    p = np.zeros(rows, dtype=np.uint32)
    p[T:4 * T] = 1                                                   # tiles 1..3 whole; no head inside tiles 2 and 3
    p[4 * T:] = 2                                                    # the last partition: one row
    o = np.arange(rows, dtype=np.int64)
    x = values(rng, rows, np.int64)
    x[T] = np.iinfo(np.int64).max                                    # the running max has to carry this through the head-less tiles
    x[4 * T - 1] = np.iinfo(np.int64).min                            # and the backward min this one
    Case(ch, ctx, [p], [o], rows).check_every_function(x, [None, WHOLE, RUNNING, AROUND, AHEAD, PEERS])


def test_a_peer_group_crosses_a_tile_without_a_head(ch, ctx, T):
    rows = 4 * T + 1
    rng = np.random.Generator(np.random.PCG64(3))
    p = np.zeros(rows, dtype=np.uint8)
    o = np.zeros(rows, dtype=np.float32)
    o[T:4 * T] = 1.5
    o[4 * T:] = 2.5
    Case(ch, ctx, [p], [o], rows).check_every_function(values(rng, rows, np.int16), [None, WHOLE, PEERS, (R.RANGE, R.CURRENT_ROW, 0, R.UNBOUNDED_FOLLOWING, 0)])


def test_the_one_workgroup_pass_loops_twice(ch, ctx, T):
    from clickhouse_amd import window
    G = window.PASS_TILES
    rows = T * G + T + 5
    rng = np.random.Generator(np.random.PCG64(4))
    part = rng.random(rows) < 1.0 / 50000
    part[T * G - 3 * T:T * G + T + 3] = False                        # one partition reaches from the first pass's tiles into the second's
    part[0] = part[rows - 1] = True
    peer = part | (rng.random(rows) < 0.3)
    peer[T * G - 2 * T:T * G + 7] = False                            # and so does one peer group
    p = np.cumsum(part).astype(np.uint32)
    o = np.cumsum(peer).astype(np.int64)
    x = rng.integers(-2**62, 2**62, size=rows, dtype=np.int64)
    case = Case(ch, ctx, [p], [o], rows)
    case.check(R.RANK)
    case.check(R.SUM, (R.ROWS, R.OFFSET_PRECEDING, 3, R.OFFSET_FOLLOWING, 1), x)
    assert case.win.counts() == (rows, int(part.sum()), int(peer.sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# random layouts: every function over every frame family
# ---------------------------------------------------------------------------------------------------------------------------------
RANDOM_ROWS = 6000


@pytest.fixture(scope="module")
def random_case(ch, ctx):
    rng = np.random.Generator(np.random.PCG64(5))
    p, o = R.geometric_layout(rng, RANDOM_ROWS, 40.0)
    return Case(ch, ctx, [p], [o], RANDOM_ROWS), values(rng, RANDOM_ROWS, np.int64), values(rng, RANDOM_ROWS, np.float64)


OFFSETS = (0, 1, 7, RANDOM_ROWS + 1)


def family_frames():
    seen = []
    for k in OFFSETS:
        for m in OFFSETS:
            for f in R.frame_families(k, m):
                if f not in seen:
                    seen.append(f)
    return seen


@pytest.mark.parametrize("function", range(12))
def test_every_function_over_every_frame_family(random_case, function):
    case, xi, xf = random_case
    if function in (R.ROW_NUMBER, R.RANK, R.DENSE_RANK):
        case.check(function)
        return
    frames = family_frames()
    assert len(frames) > 40
    for frame in frames:
        if function == R.COUNT:
            case.check(function, frame)
        elif function in (R.SUM, R.AVG):
            case.check(function, frame, xi)
        elif function in (R.MIN, R.MAX):
            if R.frame_serves_extremum(frame):
                case.check(function, frame, xi)
                case.check(function, frame, xf)
        elif function in (R.FIRST_VALUE, R.LAST_VALUE):
            case.check(function, frame, xf)
        else:
            for offset in OFFSETS + (2**64 - 1,):
                case.check(function, frame, xi, offset, -5)


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=[np.dtype(d).name for d in ALL_DTYPES])
def test_every_argument_type_with_extremes_at_partition_edges(ch, ctx, dtype):
    rows = 5000
    rng = np.random.Generator(np.random.PCG64(6))
    p, o = R.geometric_layout(rng, rows, 30.0)
    x = values(rng, rows, dtype)
    dt = np.dtype(dtype)
    special = [NAN, -NAN, 0.0, -0.0, np.inf, -np.inf] if dt.kind == "f" else [np.iinfo(dt).min, np.iinfo(dt).max, 0]
    heads = np.flatnonzero(R.heads_fast([p], [], rows)[0])
    for n, h in enumerate(heads):                                    # the first and the last row of every partition
        x[h] = special[n % len(special)]
        x[h - 1] = special[(n + 1) % len(special)]
    case = Case(ch, ctx, [p], [o], rows)
    for function in (R.MIN, R.MAX):
        for frame in (None, WHOLE, RUNNING, AHEAD, (R.ROWS, R.OFFSET_FOLLOWING, 2, R.UNBOUNDED_FOLLOWING, 0), (R.ROWS, R.UNBOUNDED_PRECEDING, 0, R.OFFSET_PRECEDING, 1)):
            case.check(function, frame, x)
    for function in (R.FIRST_VALUE, R.LAST_VALUE):
        for frame in (None, AROUND, PEERS, (R.ROWS, R.OFFSET_FOLLOWING, 1, R.OFFSET_FOLLOWING, 2)):
            case.check(function, frame, x)
    default = -NAN if dt.kind == "f" else np.iinfo(dt).min
    for function in (R.LAG_IN_FRAME, R.LEAD_IN_FRAME):
        for offset in (0, 1, 3):
            case.check(function, WHOLE, x, offset, default)
        case.check(function, AROUND, x, 2, default)


@pytest.mark.parametrize("dtype", [np.int64, np.uint64, np.int8, np.uint16])
def test_sums_wrap_around(ch, ctx, dtype):
    rows = 5000
    rng = np.random.Generator(np.random.PCG64(7))
    p, o = R.geometric_layout(rng, rows, 60.0)
    info = np.iinfo(dtype)
    x = rng.choice(np.array([info.min, info.max, info.max - 1, 1], dtype=dtype), size=rows)
    case = Case(ch, ctx, [p], [o], rows)
    for frame in (None, WHOLE, RUNNING, AROUND, AHEAD, (R.ROWS, R.OFFSET_PRECEDING, 2, R.OFFSET_PRECEDING, 1)):
        case.check(R.SUM, frame, x)
        case.check(R.AVG, frame, x)


def test_two_partition_columns_and_a_float_order_column(ch, ctx):
    rows = 3000
    rng = np.random.Generator(np.random.PCG64(8))
    a = np.sort(rng.integers(0, 6, size=rows)).astype(np.uint8)
    b = np.zeros(rows, dtype=np.int64)
    for v in range(6):                                               # within one value of a: b in runs, so that either column starts partitions
        idx = np.flatnonzero(a == v)
        b[idx] = np.sort(rng.integers(-3, 3, size=len(idx))) * 2**40
    o = np.repeat(rng.choice(np.array([0.0, -0.0, NAN, -NAN, 1.0, np.inf], dtype=np.float64), size=rows), rng.integers(1, 4, size=rows))[:rows]
    case = Case(ch, ctx, [a, b], [o], rows)
    case.check_every_function(values(rng, rows, np.int32), [None, PEERS, WHOLE])
    parts, peers = R.heads_fast([a, b], [o], rows)
    assert case.win.counts() == (rows, int(parts.sum()), int(peers.sum())) and parts.sum() > 20 and peers.sum() > parts.sum()
    # zeros of either sign are peers and so are NaNs of either sign: pinned on six rows as well
    six = np.array([0.0, -0.0, NAN, -NAN, 1.0, 1.0], dtype=np.float64)
    w = ch.Window([], [six], ctx=ctx)
    assert w.rank().tolist() == [1, 1, 3, 3, 5, 5] and w.counts() == (6, 1, 3)


@pytest.mark.parametrize("rows", [1, 2500])
def test_no_partition_and_no_order_columns(ch, ctx, rows):
    rng = np.random.Generator(np.random.PCG64(9))
    case = Case(ch, ctx, [], [], rows)
    case.check_every_function(values(rng, rows, np.uint32), [None, AROUND, AHEAD])
    assert case.win.counts() == (rows, 1, 1)
    assert case.win.count().tolist() == [rows] * rows                # all rows are peers: the default frame is the whole input


# ---------------------------------------------------------------------------------------------------------------------------------
# one handle, many calls; errors
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True], ids=["ranks-first", "frames-first"])
def test_one_handle_serves_eight_calls_in_either_order(ch, ctx, reverse):
    rows = 5000
    rng = np.random.Generator(np.random.PCG64(10))
    p, o = R.geometric_layout(rng, rows, 25.0)
    x = values(rng, rows, np.int64)
    calls = [(R.RANK, None, None), (R.ROW_NUMBER, None, None), (R.DENSE_RANK, None, None), (R.SUM, RUNNING, x), (R.COUNT, None, None),
             (R.MIN, AHEAD, x), (R.LAST_VALUE, PEERS, x), (R.LEAD_IN_FRAME, (R.ROWS, R.OFFSET_FOLLOWING, 1, R.OFFSET_FOLLOWING, 4), x)]
    case = Case(ch, ctx, [p], [o], rows)
    for function, frame, arg in (reversed(calls) if reverse else calls):
        case.check(function, frame, arg, 2, 9)
    for function, frame, arg in calls:                               # and again, from the cached bounds
        case.check(function, frame, arg, 2, 9)
    parts, peers = R.heads_fast([p], [o], rows)
    assert case.win.counts() == (rows, int(parts.sum()), int(peers.sum()))


def test_errors_leave_the_handle_usable(ch, ctx):
    K = ch._capi
    rows = 3000
    rng = np.random.Generator(np.random.PCG64(11))
    p, o = R.geometric_layout(rng, rows, 25.0)
    xi, xf = values(rng, rows, np.int64), values(rng, rows, np.float64)
    case = Case(ch, ctx, [p], [o], rows)
    w = case.win

    def fails(code, call):
        with pytest.raises(K.ChgpuError) as e:
            call()
        assert e.value.code == code, e.value
        case.check(R.SUM, AROUND, xi)                                # a second call still works
        case.check(R.MAX, WHOLE, xf)

    fails(K.ERR_NOT_IMPLEMENTED, lambda: w.sum(xi, ch.Frame.range(ch.preceding(1), ch.CURRENT_ROW)))
    fails(K.ERR_NOT_IMPLEMENTED, lambda: w.count(ch.Frame.range(ch.CURRENT_ROW, ch.following(2))))
    fails(K.ERR_NOT_IMPLEMENTED, lambda: w.sum(xf, to_frame(ch, WHOLE)))
    fails(K.ERR_NOT_IMPLEMENTED, lambda: w.avg(xf.astype(np.float32)))
    fails(K.ERR_NOT_IMPLEMENTED, lambda: w.min(xi, to_frame(ch, AROUND)))
    fails(K.ERR_NOT_IMPLEMENTED, lambda: w.max(xi, to_frame(ch, (R.ROWS, R.CURRENT_ROW, 0, R.CURRENT_ROW, 0))))

    def raw(function, frame, col, out=True):
        res = C.c_void_p()
        rc = K.lib().chgpu_window_evaluate(w._h, function, C.byref(frame) if frame is not None else None, col._h if col is not None else None, 1, 0,
                                           C.byref(res) if out else None)
        assert not res.value or rc == K.OK
        K.check(rc)
        ch.Column(ctx, res).free()

    xcol, short = ctx.upload(xi), ctx.upload(xi[:-1])
    illegal = [K.WindowFrame(K.FRAME_ROWS, K.BOUND_CURRENT_ROW, K.BOUND_OFFSET_PRECEDING, 0, 0, 1),
               K.WindowFrame(K.FRAME_ROWS, K.BOUND_OFFSET_FOLLOWING, K.BOUND_CURRENT_ROW, 0, 1, 0),
               K.WindowFrame(K.FRAME_ROWS, K.BOUND_OFFSET_PRECEDING, K.BOUND_OFFSET_PRECEDING, 0, 1, 2),
               K.WindowFrame(K.FRAME_ROWS, K.BOUND_OFFSET_FOLLOWING, K.BOUND_OFFSET_FOLLOWING, 0, 2, 1),
               K.WindowFrame(K.FRAME_RANGE, K.BOUND_UNBOUNDED_FOLLOWING, K.BOUND_UNBOUNDED_FOLLOWING, 0, 0, 0),
               K.WindowFrame(K.FRAME_ROWS, K.BOUND_UNBOUNDED_PRECEDING, K.BOUND_UNBOUNDED_PRECEDING, 0, 0, 0),
               K.WindowFrame(7, K.BOUND_UNBOUNDED_PRECEDING, K.BOUND_CURRENT_ROW, 0, 0, 0)]
    for frame in illegal:
        fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, frame, xcol))
    fails(K.ERR_SIZES_MISMATCH, lambda: raw(K.WIN_SUM, None, short))
    fails(K.ERR_SIZES_MISMATCH, lambda: raw(K.WIN_LAG_IN_FRAME, None, short))
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, None, None))
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_RANK, None, xcol))
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(12, None, xcol))
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_RANK, None, None, out=False))
    raw(K.WIN_RANK, illegal[0], None)                                # the rank functions do not look at the frame

    h = C.c_void_p()
    pcol = ctx.upload(p)
    arr = (C.c_void_p * 1)(short._h)
    with pytest.raises(K.ChgpuError) as e:
        K.check(K.lib().chgpu_window_create(ctx._h, (C.c_void_p * 1)(pcol._h), 1, arr, 1, rows, C.byref(h)))
    assert e.value.code == K.ERR_SIZES_MISMATCH and not h.value
    with pytest.raises(K.ChgpuError) as e:
        K.check(K.lib().chgpu_window_create(ctx._h, (C.c_void_p * 9)(*[pcol._h] * 9), 9, None, 0, rows, C.byref(h)))
    assert e.value.code == K.ERR_BAD_ARGUMENTS and not h.value
    with pytest.raises(K.ChgpuError) as e:
        K.check(K.lib().chgpu_window_create(ctx._h, None, 0, None, 0, 2**32, C.byref(h)))
    assert e.value.code == K.ERR_NOT_IMPLEMENTED and not h.value


# ---------------------------------------------------------------------------------------------------------------------------------
# behind the device sort
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sort_block_then_window_equals_the_reference_over_a_stable_sort(ch, ctx):
    rows = 20000
    rng = np.random.Generator(np.random.PCG64(12))
    k = rng.integers(0, 300, size=rows).astype(np.uint32)
    t = rng.integers(-50, 50, size=rows).astype(np.int64)
    x = values(rng, rows, np.int64)
    sorted_cols, _ = ch.sort_block([ctx.upload(k), ctx.upload(t), ctx.upload(x)], [(0, False, 1), (1, False, 1)])
    order = np.lexsort((t, k))                                       # stable, k most significant
    ks, ts, xs = k[order], t[order], x[order]
    assert np.array_equal(sorted_cols[2].numpy(), xs)
    w = ch.Window([sorted_cols[0]], [sorted_cols[1]])
    assert w.ctx is ctx
    sliding = (R.ROWS, R.OFFSET_PRECEDING, 9, R.CURRENT_ROW, 0)
    assert R.same_bits(w.row_number(), R.window_fast(R.ROW_NUMBER, [ks], [ts], rows))
    assert R.same_bits(w.rank(), R.window_fast(R.RANK, [ks], [ts], rows))
    assert R.same_bits(w.dense_rank(), R.window_fast(R.DENSE_RANK, [ks], [ts], rows))
    assert R.same_bits(w.sum(sorted_cols[2], to_frame(ch, RUNNING)), R.window_fast(R.SUM, [ks], [ts], rows, RUNNING, xs))
    assert R.same_bits(w.sum(sorted_cols[2], to_frame(ch, sliding)), R.window_fast(R.SUM, [ks], [ts], rows, sliding, xs))
    assert R.same_avg(w.avg(sorted_cols[2]), R.window_fast(R.AVG, [ks], [ts], rows, None, xs))
    assert R.same_bits(w.max(sorted_cols[2], to_frame(ch, WHOLE)), R.window_fast(R.MAX, [ks], [ts], rows, WHOLE, xs))
    assert R.same_bits(w.lag_in_frame(sorted_cols[2], 1, -1, to_frame(ch, WHOLE)),
                       R.window_fast(R.LAG_IN_FRAME, [ks], [ts], rows, WHOLE, xs, offset=1, default=np.int64(-1)))
    parts, peers = R.heads_fast([ks], [ts], rows)
    assert w.counts() == (rows, int(parts.sum()), int(peers.sum()))
