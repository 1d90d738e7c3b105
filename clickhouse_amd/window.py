"""Window functions over a sorted block over the C ABI (WindowTransform, src/Processors/Transforms/WindowTransform.cpp; the frames of
src/Interpreters/WindowDescription.h): one Window == one window definition, `OVER (PARTITION BY .. ORDER BY ..)`, over the WHOLE sorted
input as sort_block leaves it.  The handle keeps what it derives from the key columns (partition and peer-group bounds, built on first
use), not the keys; every method is one function OVER that window with its own frame."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from .columns import TAG_OF, Column, Context

TILE = 2048         # T: rows of one scan tile (WIN_TILE of csrc/window_host.h)
PASS_TILES = 1024   # G: tile partials one pass of the one-workgroup kernel covers (WIN_PASS)
MAX_KEYS = 8
MAX_ROWS = 2**32 - 1
_U64_MAX = 2**64 - 1


class _Bound:
    def __init__(self, kind, offset=0, name=""):
        self.kind, self.offset, self.name = kind, offset, name

    def __repr__(self):
        return self.name


UNBOUNDED = _Bound(None, 0, "UNBOUNDED")   # PRECEDING as a frame's begin, FOLLOWING as its end
CURRENT_ROW = _Bound(K.BOUND_CURRENT_ROW, 0, "CURRENT_ROW")


def _offset(k):
    k = int(k)
    if not 0 <= k <= _U64_MAX:
        raise ValueError(f"frame offset {k!r} is not a UInt64")
    return k


def preceding(k):
    return _Bound(K.BOUND_OFFSET_PRECEDING, _offset(k), f"preceding({k})")


def following(k):
    return _Bound(K.BOUND_OFFSET_FOLLOWING, _offset(k), f"following({k})")


class Frame:
    """ROWS | RANGE BETWEEN begin AND end.  Illegal frames (WindowFrame::checkValid) raise ValueError here.  Window's own methods answer
    a RANGE frame with an offset with NOT_IMPLEMENTED; Window.over(frame, order=...) serves it."""

    def __init__(self, type, begin, end):
        if type not in (K.FRAME_ROWS, K.FRAME_RANGE):
            raise ValueError(f"unknown frame type {type!r}")
        if not isinstance(begin, _Bound) or not isinstance(end, _Bound):
            raise ValueError("frame bounds are UNBOUNDED, CURRENT_ROW, preceding(k) or following(k)")
        b = K.BOUND_UNBOUNDED_PRECEDING if begin is UNBOUNDED else begin.kind
        e = K.BOUND_UNBOUNDED_FOLLOWING if end is UNBOUNDED else end.kind
        if b == K.BOUND_CURRENT_ROW and e == K.BOUND_OFFSET_PRECEDING:
            raise ValueError("frame begins at the current row and ends before it")
        if b == K.BOUND_OFFSET_FOLLOWING and e in (K.BOUND_CURRENT_ROW, K.BOUND_OFFSET_PRECEDING):
            raise ValueError("frame begins after the current row and ends at or before it")
        if b == e == K.BOUND_OFFSET_PRECEDING and begin.offset < end.offset:
            raise ValueError("frame begin is closer to the current row than its end (both PRECEDING)")
        if b == e == K.BOUND_OFFSET_FOLLOWING and begin.offset > end.offset:
            raise ValueError("frame begin is further from the current row than its end (both FOLLOWING)")
        self.type, self.begin_kind, self.end_kind = type, b, e
        self.begin_offset, self.end_offset = begin.offset, end.offset

    @classmethod
    def rows(cls, begin, end):
        return cls(K.FRAME_ROWS, begin, end)

    @classmethod
    def range(cls, begin, end):
        return cls(K.FRAME_RANGE, begin, end)

    def _c(self):
        return K.WindowFrame(self.type, self.begin_kind, self.end_kind, 0, self.begin_offset, self.end_offset)

    def __repr__(self):
        return f"Frame({'ROWS' if self.type == K.FRAME_ROWS else 'RANGE'}, {self.begin_kind}:{self.begin_offset}, {self.end_kind}:{self.end_offset})"


_INT_TAGS = (K.I64, K.U32, K.U64, K.U8, K.I32, K.U16, K.I16, K.I8)


def _tag_of(x, what):
    if isinstance(x, Column):
        return x.tag
    try:
        return TAG_OF[np.asarray(x).dtype]
    except (KeyError, TypeError):
        raise ValueError(f"{what} dtype {getattr(x, 'dtype', type(x))!r} is not one of the column types") from None


def default_bits(tag: int, value) -> int:
    """a lag / lead default as the 64 bits the C ABI takes: the value in the argument's type, zero-extended"""
    from .columns import scalar_bits
    return scalar_bits(tag, value)


def _evaluate(window: "Window", function: int, frame, x, offset: int, default, entry) -> Column:
    """What both evaluate_column methods do: the argument checks, the lag / lead default bits, the upload and the call.  `entry` is the
    caller's entry point, called only after the checks: entry(frame pointer or None, argument handle or None, offset, default bits,
    pointer to the result handle) -> return code."""
    takes_arg = function >= K.WIN_SUM
    if takes_arg != (x is not None):
        raise ValueError("the function takes an argument column" if takes_arg else "the function takes no argument column")
    bits = 0
    if takes_arg:
        tag = _tag_of(x, "argument")
        if len(x) != window.rows:
            raise ValueError(f"the argument has {len(x)} rows, the window {window.rows}")
        offset = _offset(offset)
        if function in (K.WIN_LAG_IN_FRAME, K.WIN_LEAD_IN_FRAME):
            bits = default_bits(tag, default)
        x = window.ctx.column(x)
    out = C.c_void_p()
    fc = frame._c() if frame is not None else None
    K.check(entry(C.byref(fc) if fc is not None else None, x._h if x is not None else None, offset, bits, C.byref(out)))
    return Column(window.ctx, out)


class Window:
    def __init__(self, partition_by=(), order_by=(), ctx: Context | None = None, rows: int | None = None):
        """partition_by / order_by: sequences of Columns / arrays, 0 to 8 each, already sorted by (partition_by, order_by).  rows is
        only needed when both are empty."""
        partition_by, order_by = list(partition_by), list(order_by)
        if len(partition_by) > MAX_KEYS or len(order_by) > MAX_KEYS:
            raise ValueError(f"at most {MAX_KEYS} partition and {MAX_KEYS} order columns")
        for c in partition_by:
            _tag_of(c, "partition key")
        for c in order_by:
            _tag_of(c, "order key")
        keys = partition_by + order_by
        if rows is None:
            if not keys:
                raise ValueError("a window without key columns needs rows=")
            rows = len(keys[0])
        if any(len(c) != rows for c in keys):
            raise ValueError("key columns of different lengths")
        if not 0 <= rows <= MAX_ROWS:
            raise ValueError(f"{rows} rows: a window takes at most {MAX_ROWS}")
        self.rows = int(rows)
        if ctx is None:
            ctx = next((c.ctx for c in keys if isinstance(c, Column)), None) or Context(0)
        self.ctx = ctx
        p = [ctx.column(c) for c in partition_by]   # (held until create returns: the handle keeps no reference to them)
        o = [ctx.column(c) for c in order_by]
        pa = (C.c_void_p * max(1, len(p)))(*[c._h for c in p])
        oa = (C.c_void_p * max(1, len(o)))(*[c._h for c in o])
        h = C.c_void_p()
        K.check(K.lib().chgpu_window_create(ctx._live(), pa, len(p), oa, len(o), self.rows, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            K.lib().chgpu_window_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self):
        """-> (rows, partitions, peer groups)"""
        r, p, g = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        K.check(K.lib().chgpu_window_counts(self._h, C.byref(r), C.byref(p), C.byref(g)))
        return int(r.value), int(p.value), int(g.value)

    def evaluate_column(self, function: int, frame: Frame | None = None, x=None, offset: int = 0, default=0) -> Column:
        """chgpu_window_evaluate -> the result Column resident in HBM"""
        if frame is not None and not isinstance(frame, Frame):
            raise ValueError("frame must be a Frame or None (the default frame)")
        return _evaluate(self, function, frame, x, offset, default, lambda fc, *rest: K.lib().chgpu_window_evaluate(self._h, function, fc, *rest))

    def over(self, frame: Frame | None = None, order=None, descending: bool = False) -> "FramedWindow":
        """this window with one frame, served by chgpu_window_evaluate_framed: every frame the methods below take, min / max over any
        of them, and RANGE frames with offsets -- those need `order`, the window's one ORDER BY column, and its direction"""
        return FramedWindow(self, frame, order, descending)

    def _eval(self, function, frame=None, x=None, offset=0, default=0):
        return self.evaluate_column(function, frame, x, offset, default).numpy()

    def row_number(self):
        return self._eval(K.WIN_ROW_NUMBER)

    def rank(self):
        return self._eval(K.WIN_RANK)

    def dense_rank(self):
        return self._eval(K.WIN_DENSE_RANK)

    def count(self, frame: Frame | None = None):
        return self._eval(K.WIN_COUNT, frame)

    def sum(self, x, frame: Frame | None = None):
        """integer arguments; Int64 / UInt64 wrap-around like SumSimple"""
        return self._eval(K.WIN_SUM, frame, x)

    def avg(self, x, frame: Frame | None = None):
        return self._eval(K.WIN_AVG, frame, x)

    def min(self, x, frame: Frame | None = None):
        """the frame must begin UNBOUNDED or end UNBOUNDED (Window.over(frame).min(x) takes any frame)"""
        return self._eval(K.WIN_MIN, frame, x)

    def max(self, x, frame: Frame | None = None):
        return self._eval(K.WIN_MAX, frame, x)

    def first_value(self, x, frame: Frame | None = None):
        return self._eval(K.WIN_FIRST_VALUE, frame, x)

    def last_value(self, x, frame: Frame | None = None):
        return self._eval(K.WIN_LAST_VALUE, frame, x)

    def lag_in_frame(self, x, offset: int = 1, default=0, frame: Frame | None = None):
        return self._eval(K.WIN_LAG_IN_FRAME, frame, x, offset, default)

    def lead_in_frame(self, x, offset: int = 1, default=0, frame: Frame | None = None):
        return self._eval(K.WIN_LEAD_IN_FRAME, frame, x, offset, default)


class FramedWindow:
    """Window.over(frame, order, descending): one function per method over that frame through chgpu_window_evaluate_framed.  A RANGE
    frame with an offset takes `order` (an integer column of the window's length, the one it was created with) -- checked here, before
    the library is touched; any other frame takes none."""

    def __init__(self, window: Window, frame: Frame | None = None, order=None, descending: bool = False):
        if frame is not None and not isinstance(frame, Frame):
            raise ValueError("frame must be a Frame or None (the default frame)")
        offsets = (K.BOUND_OFFSET_PRECEDING, K.BOUND_OFFSET_FOLLOWING)
        searched = frame is not None and frame.type == K.FRAME_RANGE and (frame.begin_kind in offsets or frame.end_kind in offsets)
        if searched and order is None:
            raise ValueError("a RANGE frame with an offset needs order=, the window's ORDER BY column")
        if not searched and order is not None:
            raise ValueError("order= is taken only with a RANGE frame that has an offset")
        if order is not None:
            if _tag_of(order, "order key") not in _INT_TAGS:
                raise ValueError("a RANGE frame with an offset takes an integer ORDER BY column, not Float32 / Float64")
            if len(order) != window.rows:
                raise ValueError(f"the order column has {len(order)} rows, the window {window.rows}")
            order = window.ctx.column(order)
        self.window, self.frame, self.order, self.descending = window, frame, order, bool(descending)

    def evaluate_column(self, function: int, x=None, offset: int = 0, default=0) -> Column:
        """chgpu_window_evaluate_framed -> the result Column resident in HBM"""
        w, order = self.window, self.order._h if self.order is not None else None
        return _evaluate(w, function, self.frame, x, offset, default,
                         lambda fc, *rest: K.lib().chgpu_window_evaluate_framed(w._h, function, fc, order, 1 if self.descending else 0, *rest))

    def _eval(self, function, x=None, offset=0, default=0):
        return self.evaluate_column(function, x, offset, default).numpy()

    def count(self):
        return self._eval(K.WIN_COUNT)

    def sum(self, x):
        """integer arguments; Int64 / UInt64 wrap-around like SumSimple"""
        return self._eval(K.WIN_SUM, x)

    def avg(self, x):
        return self._eval(K.WIN_AVG, x)

    def min(self, x):
        """any legal frame"""
        return self._eval(K.WIN_MIN, x)

    def max(self, x):
        return self._eval(K.WIN_MAX, x)

    def first_value(self, x):
        return self._eval(K.WIN_FIRST_VALUE, x)

    def last_value(self, x):
        return self._eval(K.WIN_LAST_VALUE, x)

    def lag_in_frame(self, x, offset: int = 1, default=0):
        return self._eval(K.WIN_LAG_IN_FRAME, x, offset, default)

    def lead_in_frame(self, x, offset: int = 1, default=0):
        return self._eval(K.WIN_LEAD_IN_FRAME, x, offset, default)
