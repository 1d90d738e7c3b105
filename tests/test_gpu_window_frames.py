"""chgpu_window_evaluate_framed on the device against tests/window_frames_ref.py, bit for bit (a NaN cell of an avg column is compared as
NaN): min / max over frames bounded on both sides, RANGE frames with offsets for every function that reads a frame, agreement with the
old entry wherever that serves the call, and the refusals.

T is the scan tile; a block of the general min / max is 64 rows.  The shapes are the smallest at which each mechanism can break: sizes
around the block and the tile, frames whose width is around one, two and three blocks (so that a frame lies in one block, touches two, or
has whole blocks between that the sparse table answers), partition heads exactly at block and tile edges, and one input of 64 T + 65 rows
whose table of 2049 blocks crosses a workgroup of the table kernels and has eleven levels.  Inputs of up to 65 rows are checked against
the per-row reference, larger ones against the fast form (test_window_frames_ref.py holds the two together)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_frames_ref as F  # noqa: E402
import window_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
U64 = 2**64 - 1
WHOLE = (R.ROWS, R.UNBOUNDED_PRECEDING, 0, R.UNBOUNDED_FOLLOWING, 0)
RUNNING = (R.ROWS, R.UNBOUNDED_PRECEDING, 0, R.CURRENT_ROW, 0)
AHEAD = (R.ROWS, R.CURRENT_ROW, 0, R.UNBOUNDED_FOLLOWING, 0)
AROUND = (R.ROWS, R.OFFSET_PRECEDING, 3, R.OFFSET_FOLLOWING, 1)
PEERS = (R.RANGE, R.CURRENT_ROW, 0, R.CURRENT_ROW, 0)
ALL_DTYPES = (np.int64, np.uint32, np.uint64, np.float64, np.uint8, np.int32, np.uint16, np.int16, np.int8, np.float32)
ORDER_DTYPES = (np.int64, np.uint64, np.int32, np.uint32, np.int16, np.uint16, np.int8, np.uint8)
WIDTHS = (0, 1, 62, 63, 64, 65, 127, 128, 191, 1000, U64)            # k and m of ROWS k PRECEDING .. m FOLLOWING


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
    return window.TILE


def to_frame(ch, f):
    if f is None:
        return None

    def bound(kind, off):
        if kind in (R.UNBOUNDED_PRECEDING, R.UNBOUNDED_FOLLOWING):
            return ch.UNBOUNDED
        return ch.CURRENT_ROW if kind == R.CURRENT_ROW else ch.preceding(off) if kind == R.OFFSET_PRECEDING else ch.following(off)
    return ch.Frame(f[0], bound(f[1], f[2]), bound(f[3], f[4]))


def _first_difference(got, want):
    a, b = got.view(f"u{got.dtype.itemsize}"), want.view(f"u{want.dtype.itemsize}")
    if a.shape != b.shape:
        return (a.shape, b.shape)
    d = np.flatnonzero(a != b)
    return None if not len(d) else (int(d[0]), got[d[0]], want[d[0]], len(d))


class Case:
    """one window over host columns, the device handle beside them; descending: the direction of the one order column"""

    def __init__(self, ch, ctx, part_cols, order_cols, rows, descending=False):
        self.ch, self.ctx, self.p, self.o, self.rows, self.descending = ch, ctx, list(part_cols), list(order_cols), rows, descending
        self.win = ch.Window(self.p, self.o, ctx=ctx, rows=rows)
        self.slow = rows <= 65
        self._dev = {}
        self._order = None

    def column(self, x):
        held = self._dev.get(id(x))                      # (the array is held beside its column: a freed array's id may come again)
        if held is None:
            held = self._dev[id(x)] = (x, self.ctx.upload(x))
        return held[1]

    def over(self, frame):
        order = None
        if F.has_range_offset(frame):
            if self._order is None:
                self._order = self.ctx.upload(self.o[0])
            order = self._order
        return self.win.over(to_frame(self.ch, frame), order=order, descending=self.descending)

    def check(self, function, frame=None, x=None, offset=1, default=0):
        if x is not None:
            default = x.dtype.type(default)
        got = self.over(frame).evaluate_column(function, None if x is None else self.column(x), offset, default).numpy()
        ref = F.window_slow if self.slow else F.window_fast
        want = ref(function, self.p, self.o, self.rows, frame, x, offset=offset, default=default, descending=self.descending)
        same = R.same_avg if function == R.AVG else R.same_bits
        assert got.dtype == want.dtype and same(got, want), (function, frame, None if x is None else x.dtype, offset, _first_difference(got, want))

    def check_extrema(self, x, frames):
        for frame in frames:
            self.check(R.MIN, frame, x)
            self.check(R.MAX, frame, x)


def values(rng, rows, dtype=np.int64):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return rng.standard_normal(rows).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=rows, dtype=dt, endpoint=True)


def width_pairs(shift):
    """every width of WIDTHS once as k and once as m"""
    return [(WIDTHS[i], WIDTHS[(i + shift) % len(WIDTHS)]) for i in range(len(WIDTHS))]


def extremum_frames(pairs):
    seen = []
    for k, m in pairs:
        seen += [f for f in F.two_sided_frames(k, m) if f not in seen]
    return seen + [PEERS]


# ---------------------------------------------------------------------------------------------------------------------------------
# min / max over any frame
# ---------------------------------------------------------------------------------------------------------------------------------
def sizes(T):
    return [1, 2, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 2 * T + 65]


@pytest.mark.parametrize("own_partition", [False, True], ids=["one-partition", "row-per-partition"])
@pytest.mark.parametrize("size_index", range(12))
def test_extrema_at_sizes_around_the_block_and_the_tile(ch, ctx, T, size_index, own_partition):
    rows = sizes(T)[size_index]
    rng = np.random.Generator(np.random.PCG64(200 + size_index))
    p = np.arange(rows, dtype=np.uint32) if own_partition else np.full(rows, 7, dtype=np.uint32)
    o = (np.arange(rows, dtype=np.int64) // 3) if not own_partition else np.zeros(rows, dtype=np.int64)
    case = Case(ch, ctx, [p], [o], rows)
    frames = extremum_frames(width_pairs(3 + size_index % 5))
    assert len(frames) > 40
    case.check_extrema(values(rng, rows, np.int32), frames[:12] if own_partition else frames)


def test_every_pair_of_widths_over_one_partition(ch, ctx, T):
    rows = 2 * T + 65
    rng = np.random.Generator(np.random.PCG64(20))
    case = Case(ch, ctx, [np.zeros(rows, dtype=np.uint8)], [np.arange(rows, dtype=np.int64)], rows)
    x = rng.integers(0, 3, size=rows).astype(np.int64)               # values from {0, 1, 2}: ties in every block
    n = 0
    for k in WIDTHS:
        for m in WIDTHS:
            case.check(R.MIN if n % 2 else R.MAX, (R.ROWS, R.OFFSET_PRECEDING, k, R.OFFSET_FOLLOWING, m), x)
            n += 1
    assert n == 121


def test_the_table_crosses_a_workgroup_and_has_eleven_levels(ch, ctx, T):
    rows = 64 * T + 65                                               # 2049 blocks
    rng = np.random.Generator(np.random.PCG64(21))
    case = Case(ch, ctx, [np.zeros(rows, dtype=np.uint32)], [np.arange(rows, dtype=np.int64)], rows)
    x = values(rng, rows, np.int64)
    x[64 * 1030 + 5] = np.iinfo(np.int64).max                        # the extremum of everything, in a block of the second workgroup
    case.check(R.MAX, (R.ROWS, R.OFFSET_PRECEDING, 1000, R.OFFSET_FOLLOWING, 1000), x)
    case.check(R.MIN, (R.ROWS, R.OFFSET_PRECEDING, U64, R.OFFSET_FOLLOWING, U64), x)   # every frame the whole partition: the top level


@pytest.mark.parametrize("mean", [5, 100, 3000])
def test_extrema_over_geometric_partitions(ch, ctx, T, mean):
    rows = 2 * T + 65
    rng = np.random.Generator(np.random.PCG64(22 + mean))
    p, o = R.geometric_layout(rng, rows, float(mean))
    case = Case(ch, ctx, [p], [o], rows)
    case.check_extrema(values(rng, rows, np.int64), extremum_frames(width_pairs(4))[::2])
    case.check_extrema(values(rng, rows, np.float64), extremum_frames(width_pairs(7))[1::2])


def test_partition_heads_exactly_at_block_and_tile_edges(ch, ctx, T):
    rows = 2 * T + 65
    rng = np.random.Generator(np.random.PCG64(23))
    heads = np.zeros(rows, dtype=bool)
    heads[[0, 63, 64, 65, T - 1, T, T + 1]] = True
    p = np.cumsum(heads).astype(np.uint16)
    o = (np.arange(rows) // 2).astype(np.int32)
    case = Case(ch, ctx, [p], [o], rows)
    x = values(rng, rows, np.int16)
    x[[62, 63, 64, 65, 66, T - 2, T - 1, T, T + 1, T + 2]] = [32767, -32768, 32767, -32768, 32767, -32768, 32767, -32768, 32767, -32768]
    case.check_extrema(x, extremum_frames(width_pairs(2)))


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=[np.dtype(d).name for d in ALL_DTYPES])
def test_extrema_of_every_type_and_value_shape(ch, ctx, T, dtype):
    rows = T + 65
    rng = np.random.Generator(np.random.PCG64(24))
    p, o = R.geometric_layout(rng, rows, 300.0)
    case = Case(ch, ctx, [p], [o], rows)
    dt = np.dtype(dtype)
    frames = [(R.ROWS, R.OFFSET_PRECEDING, 63, R.OFFSET_FOLLOWING, 64), (R.ROWS, R.OFFSET_PRECEDING, 200, R.OFFSET_PRECEDING, 5),
              (R.ROWS, R.OFFSET_FOLLOWING, 1, R.OFFSET_FOLLOWING, 130), (R.ROWS, R.CURRENT_ROW, 0, R.CURRENT_ROW, 0), PEERS]
    x = values(rng, rows, dtype)
    if dt.kind == "f":
        special = np.array([NAN, -NAN, 0.0, -0.0, np.inf, -np.inf], dtype=dt)
        at = rng.random(rows) < 0.2
        x[at] = rng.choice(special, size=int(at.sum()))
        zeros = np.where(rng.random(rows) < 0.5, dt.type(0.0), dt.type(-0.0)).astype(dt)   # only +0.0 and -0.0: +0.0 is above
        case.check_extrema(zeros, frames[:2])
        lo, hi = -1000, 1000
    else:
        info = np.iinfo(dt)
        at = rng.random(rows) < 0.1
        x[at] = rng.choice(np.array([info.min, info.max, 0], dtype=dt), size=int(at.sum()))
        lo, hi = max(int(info.min), -1000), min(int(info.max), 1000)
    case.check_extrema(x, frames)
    case.check_extrema(np.full(rows, x[0], dtype=dt), frames[:3])                                           # all rows equal
    ramp = (lo + np.arange(rows) % (hi - lo + 1)).astype(dt)         # strictly rising inside a block: a stack of one row
    case.check_extrema(ramp, frames[:3])
    case.check_extrema(ramp[::-1].copy(), frames[:3])                # strictly falling: a stack of 64
    case.check_extrema(rng.integers(0, 3, size=rows).astype(dt), frames[:3])


# ---------------------------------------------------------------------------------------------------------------------------------
# RANGE frames with offsets
# ---------------------------------------------------------------------------------------------------------------------------------
RANGE_OFFSETS = (0, 1, 2, 3, 2**63, U64)


def range_frames():
    """every shape of RANGE frame with every offset as k and as m"""
    seen = []
    for i, k in enumerate(RANGE_OFFSETS):
        for m in (RANGE_OFFSETS[(i + 1) % 6], RANGE_OFFSETS[(i + 4) % 6]):
            seen += [f for f in F.range_offset_frames(k, m) if f not in seen]
    return seen


def check_frame_functions(case, frames, xi, xf, rotate=True):
    """COUNT over every frame; the eight functions with an argument over every frame in turn (rotate) or all of them"""
    others = [f for f in F.FRAME_FUNCTIONS if f != R.COUNT]
    for n, frame in enumerate(frames):
        case.check(R.COUNT, frame)
        for function in ([others[(n + j) % 8] for j in range(3)] if rotate else others):
            if function in (R.SUM, R.AVG):
                case.check(function, frame, xi)
            elif function in (R.LAG_IN_FRAME, R.LEAD_IN_FRAME):
                for offset in (0, 1, 3, U64):                        # inside and outside the frame
                    case.check(function, frame, xi, offset, -5)
            else:
                case.check(function, frame, xf if n % 2 else xi)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype", ORDER_DTYPES, ids=[np.dtype(d).name for d in ORDER_DTYPES])
def test_range_offsets_over_every_order_type_and_direction(ch, ctx, T, dtype, descending):
    rows = T + 65
    rng = np.random.Generator(np.random.PCG64(30 + np.dtype(dtype).num))
    p, _ = R.geometric_layout(rng, rows, 100.0)
    part = R.heads_fast([p], [], rows)[0]
    # duplicates (a bound lands on another peer group's edge), gaps wider than the small offsets (empty FOLLOWING .. FOLLOWING frames),
    # and every partition from the type's minimum to its maximum, so that x - k and x + k leave the type on either side
    o = F.sorted_order(rng, part, dtype, descending, at_limits=True)
    case = Case(ch, ctx, [p], [o], rows, descending)
    frames = range_frames()
    assert len(frames) > 60
    counts = F.window_fast(R.COUNT, [p], [o], rows, (R.RANGE, R.OFFSET_FOLLOWING, 1, R.OFFSET_FOLLOWING, 2), descending=descending)
    assert (counts == 0).any() and (counts > 0).any()
    check_frame_functions(case, frames, values(rng, rows, np.int32), values(rng, rows, np.float64))


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_the_gallop_doubles_a_dozen_times_and_hits_the_partition_edge(ch, ctx, T, descending):
    rows = 2 * T + 65
    rng = np.random.Generator(np.random.PCG64(31))
    o = np.arange(rows, dtype=np.int64) - 1000                       # unit steps: an offset of k is k rows away
    if descending:
        o = o[::-1].copy()
    case = Case(ch, ctx, [np.zeros(rows, dtype=np.uint32)], [o], rows, descending)
    xi = values(rng, rows, np.int64)
    for k in (1, 64, 3000, 10**6):
        for frame in ((R.RANGE, R.OFFSET_PRECEDING, k, R.OFFSET_FOLLOWING, k), (R.RANGE, R.OFFSET_PRECEDING, k, R.CURRENT_ROW, 0),
                      (R.RANGE, R.OFFSET_FOLLOWING, 1, R.OFFSET_FOLLOWING, k), (R.RANGE, R.OFFSET_PRECEDING, k, R.OFFSET_PRECEDING, 1)):
            case.check(R.COUNT, frame)
            case.check(R.SUM, frame, xi)
            case.check(R.MAX, frame, xi)
    rows_frame = (R.ROWS, R.OFFSET_PRECEDING, 64, R.OFFSET_FOLLOWING, 64)
    got = case.over((R.RANGE, R.OFFSET_PRECEDING, 64, R.OFFSET_FOLLOWING, 64)).sum(case.column(xi))
    assert R.same_bits(got, case.win.sum(case.column(xi), to_frame(ch, rows_frame)))    # over unit steps RANGE k is ROWS k


@pytest.mark.parametrize("mean", [5, 3000])
def test_range_offsets_over_geometric_partitions(ch, ctx, T, mean):
    rows = 2 * T + 65
    rng = np.random.Generator(np.random.PCG64(32 + mean))
    p, o = R.geometric_layout(rng, rows, float(mean), mean_group=1.5)
    o = (o * 3 + rng.integers(0, 2, size=rows).cumsum()).astype(np.int64)   # still sorted: gaps of 0, 1, 3 and 4
    case = Case(ch, ctx, [p], [o], rows)
    frames = [f for k, m in ((1, 2), (3, 40), (500, 7), (0, 10**4)) for f in F.range_offset_frames(k, m)]
    check_frame_functions(case, frames, values(rng, rows, np.int64), values(rng, rows, np.float32))


def test_every_function_over_range_offsets_on_a_small_input(ch, ctx):
    rows = 65                                                        # against the per-row definition
    rng = np.random.Generator(np.random.PCG64(33))
    p, _ = R.geometric_layout(rng, rows, 20.0)
    part = R.heads_fast([p], [], rows)[0]
    for dtype, descending in ((np.int8, False), (np.uint64, True)):
        o = F.sorted_order(rng, part, dtype, descending, at_limits=True)
        case = Case(ch, ctx, [p], [o], rows, descending)
        assert case.slow
        check_frame_functions(case, range_frames()[::3], values(rng, rows, np.int16), values(rng, rows, np.float32), rotate=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# agreement with the old entry
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_index", range(3))
def test_over_gives_the_bits_of_the_window_methods(ch, ctx, T, rows_index):
    K = ch._capi
    rows = [65, T + 1, 2 * T + 1][rows_index]
    rng = np.random.Generator(np.random.PCG64(40 + rows_index))
    p, o = R.geometric_layout(rng, rows, 40.0)
    win = ch.Window([p], [o], ctx=ctx)
    xi, xf = ctx.upload(values(rng, rows, np.int64)), ctx.upload(values(rng, rows, np.float64))
    for frame in (WHOLE, RUNNING, AHEAD, AROUND, PEERS, None):
        f = to_frame(ch, frame)
        fw = win.over(f)
        assert R.same_bits(fw.count(), win.count(f))
        assert R.same_bits(fw.sum(xi), win.sum(xi, f)) and R.same_avg(fw.avg(xi), win.avg(xi, f))
        if R.frame_serves_extremum(frame):
            for x in (xi, xf):
                assert R.same_bits(fw.min(x), win.min(x, f)) and R.same_bits(fw.max(x), win.max(x, f))
        for x in (xi, xf):
            assert R.same_bits(fw.first_value(x), win.first_value(x, f)) and R.same_bits(fw.last_value(x), win.last_value(x, f))
            assert R.same_bits(fw.lag_in_frame(x, 2, -3), win.lag_in_frame(x, 2, -3, f))
            assert R.same_bits(fw.lead_in_frame(x, 1, 7), win.lead_in_frame(x, 1, 7, f))
        for function in (K.WIN_ROW_NUMBER, K.WIN_RANK, K.WIN_DENSE_RANK):
            assert R.same_bits(fw.evaluate_column(function).numpy(), win.evaluate_column(function).numpy())


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals and state
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(ch, ctx, T):
    K = ch._capi
    rows = T + 65
    rng = np.random.Generator(np.random.PCG64(50))
    p, o = R.geometric_layout(rng, rows, 25.0)
    xi, xf = values(rng, rows, np.int64), values(rng, rows, np.float64)
    case = Case(ch, ctx, [p], [o], rows)
    w = case.win
    week = (R.RANGE, R.OFFSET_PRECEDING, 7, R.CURRENT_ROW, 0)
    wide = (R.ROWS, R.OFFSET_PRECEDING, 70, R.OFFSET_FOLLOWING, 70)

    def fails(code, call, on=case):
        with pytest.raises(K.ChgpuError) as e:
            call()
        assert e.value.code == code, e.value
        on.check(R.MAX, wide, xf)                                    # the handle still serves: the general min / max,
        if on is case:
            on.check(R.SUM, week, xi)                                # a searched frame,
        on.check(R.COUNT, AROUND)                                    # and the old path

    def raw(function, frame, order, col, out=True, handle=w, descending=0):
        res = C.c_void_p()
        rc = K.lib().chgpu_window_evaluate_framed(handle._h, function, C.byref(frame) if frame is not None else None, order._h if order is not None else None,
                                                  descending, col._h if col is not None else None, 1, 0, C.byref(res) if out else None)
        assert not res.value or rc == K.OK
        K.check(rc)
        ch.Column(ctx, res).free()

    c_week = K.WindowFrame(K.FRAME_RANGE, K.BOUND_OFFSET_PRECEDING, K.BOUND_CURRENT_ROW, 0, 7, 0)
    c_rows = K.WindowFrame(K.FRAME_ROWS, K.BOUND_OFFSET_PRECEDING, K.BOUND_CURRENT_ROW, 0, 7, 0)
    ocol, xcol, short = ctx.upload(o), ctx.upload(xi), ctx.upload(xi[:-1])
    raw(K.WIN_SUM, c_week, ocol, xcol)                               # the served form of the calls below
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, c_week, None, xcol))                       # a RANGE offset without the order column
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, c_rows, ocol, xcol))                       # an order column with a ROWS frame,
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, None, ocol, xcol))                         # with the default frame,
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_RANK, c_week, ocol, None))                      # with a function that ignores the frame
    fails(K.ERR_BAD_ARGUMENTS, lambda: w.over(to_frame(ch, week), order=o.astype(np.int32)).count())   # not the type recorded at create
    fails(K.ERR_SIZES_MISMATCH, lambda: raw(K.WIN_SUM, c_week, short, xcol))
    fails(K.ERR_SIZES_MISMATCH, lambda: raw(K.WIN_SUM, c_week, ocol, short))
    fails(K.ERR_NOT_IMPLEMENTED, lambda: case.over(week).sum(xf))                                # float sums stay out
    fails(K.ERR_NOT_IMPLEMENTED, lambda: case.over(wide).avg(xf.astype(np.float32)))
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, c_week, ocol, None))                       # no argument
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_COUNT, c_week, ocol, xcol))                     # a surplus one
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(12, c_week, ocol, xcol))
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_COUNT, c_week, ocol, None, out=False))
    for frame in (K.WindowFrame(K.FRAME_RANGE, K.BOUND_CURRENT_ROW, K.BOUND_OFFSET_PRECEDING, 0, 0, 1),
                  K.WindowFrame(K.FRAME_RANGE, K.BOUND_OFFSET_PRECEDING, K.BOUND_OFFSET_PRECEDING, 0, 1, 2),
                  K.WindowFrame(K.FRAME_RANGE, K.BOUND_OFFSET_FOLLOWING, K.BOUND_OFFSET_FOLLOWING, 0, 2, 1),
                  K.WindowFrame(K.FRAME_ROWS, K.BOUND_OFFSET_FOLLOWING, K.BOUND_CURRENT_ROW, 0, 1, 0),
                  K.WindowFrame(7, K.BOUND_OFFSET_PRECEDING, K.BOUND_CURRENT_ROW, 0, 1, 0)):
        fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_MAX, frame, ocol, xcol))                    # illegal frames, whatever comes with them
    raw(K.WIN_RANK, c_week, None, None)                              # the rank functions do not look at the frame

    # windows with no, two and a float order column
    none = Case(ch, ctx, [p], [], rows)
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, c_week, ocol, xcol, handle=none.win), on=none)
    two = Case(ch, ctx, [p], [o, o], rows)
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, c_week, ocol, xcol, handle=two.win), on=two)
    of = o.astype(np.float64)
    floats = Case(ch, ctx, [p], [of], rows)
    fcol = ctx.upload(of)
    fails(K.ERR_NOT_IMPLEMENTED, lambda: raw(K.WIN_SUM, c_week, fcol, xcol, handle=floats.win), on=floats)
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, c_week, ocol, xcol, handle=floats.win), on=floats)   # Int64 is not what create saw
    # a float order column on a handle that would not take the column anyway: what the handle refuses comes before NOT_IMPLEMENTED
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, c_week, fcol, xcol, handle=none.win), on=none)
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, c_week, fcol, xcol, handle=two.win), on=two)
    fails(K.ERR_BAD_ARGUMENTS, lambda: raw(K.WIN_SUM, c_week, fcol, xcol))                       # w recorded Int64


def test_an_empty_input(ch, ctx):
    w = ch.Window([np.zeros(0, dtype=np.uint32)], [np.zeros(0, dtype=np.int64)], ctx=ctx)
    x = np.zeros(0, dtype=np.int16)
    assert w.over(ch.Frame.rows(ch.preceding(2), ch.following(2))).max(x).shape == (0,)
    got = w.over(ch.Frame.range(ch.preceding(2), ch.CURRENT_ROW), order=np.zeros(0, dtype=np.int64)).sum(x)
    assert got.shape == (0,) and got.dtype == np.int64
