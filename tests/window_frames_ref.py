"""Reference for chgpu_window_evaluate_framed beside tests/window_ref.py (imported, not changed): every legal frame, min / max over any of
them, and RANGE frames with offsets over one integer ORDER BY column, ascending or descending.

window_slow is the definition: a RANGE bound by a linear scan of the partition in Python integers (the contract's exact arithmetic:
x[i] - k and x[i] + k are never rounded or wrapped), the extremum by brute force over window_ref.order_key of the frame's rows.
window_fast is the same for inputs too large for the loops: np.searchsorted per partition on arrays of Python integers, and a per-row
slice extremum.  tests/test_window_frames_ref.py holds the two together and both against window_ref where that serves the frame.

A frame is window_ref's tuple (type, begin_kind, begin_offset, end_kind, end_offset), None the default frame."""
import numpy as np

import window_ref as R

OFFSETS = (R.OFFSET_PRECEDING, R.OFFSET_FOLLOWING)
FRAME_FUNCTIONS = (R.COUNT, R.SUM, R.AVG, R.MIN, R.MAX, R.FIRST_VALUE, R.LAST_VALUE, R.LAG_IN_FRAME, R.LEAD_IN_FRAME)


def has_range_offset(frame):
    return frame is not None and frame[0] == R.RANGE and (frame[1] in OFFSETS or frame[3] in OFFSETS)


def range_bound_slow(y, i, ps, pe, gs, ge, kind, k, end):
    """one bound of row i's RANGE frame; y: the partition-sorted order values as Python integers, negated when descending"""
    if kind == R.UNBOUNDED_PRECEDING:
        return ps
    if kind == R.UNBOUNDED_FOLLOWING:
        return pe
    if kind == R.CURRENT_ROW or k == 0:
        return ge if end else gs
    t = y[i] - k if kind == R.OFFSET_PRECEDING else y[i] + k
    for j in range(ps, pe):
        if (y[j] > t) if end else (y[j] >= t):
            return j
    return pe


def frames_slow(frame, partition_cols, order_cols, rows, descending=False):
    frame = R.DEFAULT_FRAME if frame is None else frame
    assert R.frame_is_legal(frame)
    part, peer = R.heads_slow(partition_cols, order_cols, rows)
    ps, pe = R.bounds_slow(part, rows)
    gs, ge = R.bounds_slow(peer, rows)
    if not has_range_offset(frame):
        both = [R.frame_slow(frame, i, ps[i], pe[i], gs[i], ge[i]) for i in range(rows)]
        return [b[0] for b in both], [b[1] for b in both]
    assert len(order_cols) == 1 and order_cols[0].dtype.kind in "iu"
    y = [-int(v) if descending else int(v) for v in order_cols[0]]
    _, b, bo, e, eo = frame
    fs = [range_bound_slow(y, i, ps[i], pe[i], gs[i], ge[i], b, bo, False) for i in range(rows)]
    fe = [range_bound_slow(y, i, ps[i], pe[i], gs[i], ge[i], e, eo, True) for i in range(rows)]
    return fs, fe


def window_slow(function, partition_cols, order_cols, rows, frame=None, x=None, offset=1, default=0, descending=False):
    if function in (R.ROW_NUMBER, R.RANK, R.DENSE_RANK):
        return R.window_slow(function, partition_cols, order_cols, rows)
    fs_all, fe_all = frames_slow(frame, partition_cols, order_cols, rows, descending)
    dt = None if x is None else x.dtype
    out = np.zeros(rows, dtype=R.result_dtype(function, dt))
    for i in range(rows):
        fs, fe = fs_all[i], fe_all[i]
        assert fs <= fe
        if function == R.COUNT:
            out[i] = fe - fs
            continue
        rows_of_frame = x[fs:fe]
        if function == R.SUM:
            out[i] = R._wrap(sum(int(v) for v in rows_of_frame), dt)
        elif function == R.AVG:
            num = R._wrap(sum(int(v) for v in rows_of_frame), dt)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[i] = np.float64(num) / np.float64(fe - fs)
        elif function in (R.MIN, R.MAX):
            if len(rows_of_frame):
                out[i] = (min if function == R.MIN else max)(rows_of_frame, key=R.order_key)
        elif function == R.FIRST_VALUE:
            if len(rows_of_frame):
                out[i] = rows_of_frame[0]
        elif function == R.LAST_VALUE:
            if len(rows_of_frame):
                out[i] = rows_of_frame[-1]
        else:
            t = i - offset if function == R.LAG_IN_FRAME else i + offset
            out[i] = x[t] if fs <= t < fe else default
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the same for larger inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def frames_fast(frame, partition_cols, order_cols, rows, descending=False):
    frame = R.DEFAULT_FRAME if frame is None else frame
    assert R.frame_is_legal(frame)
    part, peer = R.heads_fast(partition_cols, order_cols, rows)
    ps, pe = R.bounds_fast(part, rows)
    gs, ge = R.bounds_fast(peer, rows)
    if not has_range_offset(frame):
        return R.frames_fast(frame, rows, ps, pe, gs, ge)
    assert len(order_cols) == 1 and order_cols[0].dtype.kind in "iu"
    y = np.array([-int(v) if descending else int(v) for v in order_cols[0]], dtype=object)
    _, b, bo, e, eo = frame

    def bound(kind, k, end):
        if kind == R.UNBOUNDED_PRECEDING:
            return ps
        if kind == R.UNBOUNDED_FOLLOWING:
            return pe
        if kind == R.CURRENT_ROW or k == 0:
            return ge if end else gs
        out = np.empty(rows, dtype=np.int64)
        for a in np.flatnonzero(part):
            z = pe[a]
            keys = y[a:z]
            targets = keys - k if kind == R.OFFSET_PRECEDING else keys + k
            out[a:z] = a + np.searchsorted(keys, targets, side="right" if end else "left")
        return out
    return bound(b, bo, False), bound(e, eo, True)


def window_fast(function, partition_cols, order_cols, rows, frame=None, x=None, offset=1, default=0, descending=False):
    if function in (R.ROW_NUMBER, R.RANK, R.DENSE_RANK) or rows == 0:
        return R.window_fast(function, partition_cols, order_cols, rows, None, x)
    fs, fe = frames_fast(frame, partition_cols, order_cols, rows, descending)
    fs, fe = np.asarray(fs, dtype=np.int64), np.asarray(fe, dtype=np.int64)
    assert bool(np.all(fs <= fe))
    i = np.arange(rows, dtype=np.int64)
    dt = None if x is None else x.dtype
    rdt = R.result_dtype(function, dt)
    if function == R.COUNT:
        return (fe - fs).astype(rdt)
    empty = fs >= fe
    if function in (R.SUM, R.AVG):
        wide = x.astype(np.int64).view(np.uint64) if dt.kind == "i" else x.astype(np.uint64)
        p = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(wide, dtype=np.uint64)])
        s = (p[fe] - p[fs]).view(R.sum_result_dtype(dt))
        if function == R.SUM:
            return s
        with np.errstate(invalid="ignore", divide="ignore"):
            return s.astype(np.float64) / (fe - fs).astype(np.float64)
    raw = x.view(f"u{dt.itemsize}")
    if function in (R.MIN, R.MAX):
        keys = R.order_keys_fast(x)
        pick = np.argmin if function == R.MIN else np.argmax
        found = {}                                     # rows with the same frame (a whole partition, a peer group) share one slice

        def at(a, z):
            if (a, z) not in found:
                found[(a, z)] = 0 if a >= z else a + int(pick(keys[a:z]))
            return found[(a, z)]
        src = np.array([at(a, z) for a, z in zip(fs.tolist(), fe.tolist())], dtype=np.int64)
    elif function == R.FIRST_VALUE:
        src = np.where(empty, 0, fs)
    elif function == R.LAST_VALUE:
        src = np.where(empty, 0, fe - 1)
    else:
        k = min(offset, rows + 1)
        t = i - k if function == R.LAG_IN_FRAME else i + k
        empty = ~((t >= fs) & (t < fe))
        src = np.where(empty, 0, t)
        return np.where(empty, np.array([default], dtype=dt).view(f"u{dt.itemsize}")[0], raw[src]).astype(f"u{dt.itemsize}").view(dt)
    return np.where(empty, 0, raw[src]).astype(f"u{dt.itemsize}").view(dt)


def two_sided_frames(k, m):
    """the frames min / max gain here, for the offsets k, m (ordered as each family's validity asks)"""
    lo, hi = min(k, m), max(k, m)
    return [(R.ROWS, R.OFFSET_PRECEDING, k, R.OFFSET_FOLLOWING, m),
            (R.ROWS, R.OFFSET_PRECEDING, hi, R.OFFSET_PRECEDING, lo),
            (R.ROWS, R.OFFSET_FOLLOWING, lo, R.OFFSET_FOLLOWING, hi),
            (R.ROWS, R.OFFSET_PRECEDING, k, R.CURRENT_ROW, 0),
            (R.ROWS, R.CURRENT_ROW, 0, R.OFFSET_FOLLOWING, m)]


def range_offset_frames(k, m):
    """one RANGE frame with an offset of every shape, for the offsets k, m"""
    lo, hi = min(k, m), max(k, m)
    return [(R.RANGE, R.OFFSET_PRECEDING, k, R.OFFSET_FOLLOWING, m),
            (R.RANGE, R.OFFSET_PRECEDING, hi, R.OFFSET_PRECEDING, lo),
            (R.RANGE, R.OFFSET_FOLLOWING, lo, R.OFFSET_FOLLOWING, hi),
            (R.RANGE, R.OFFSET_PRECEDING, k, R.CURRENT_ROW, 0),
            (R.RANGE, R.CURRENT_ROW, 0, R.OFFSET_FOLLOWING, m),
            (R.RANGE, R.UNBOUNDED_PRECEDING, 0, R.OFFSET_FOLLOWING, m),
            (R.RANGE, R.UNBOUNDED_PRECEDING, 0, R.OFFSET_PRECEDING, k),
            (R.RANGE, R.OFFSET_PRECEDING, k, R.UNBOUNDED_FOLLOWING, 0),
            (R.RANGE, R.OFFSET_FOLLOWING, m, R.UNBOUNDED_FOLLOWING, 0)]


def sorted_order(rng, part, dtype, descending=False, step_choices=(0, 0, 1, 1, 2, 7), at_limits=False):
    """an order column of `dtype` sorted inside the partitions that `part` (bool heads) starts: steps drawn from step_choices, so there
    are duplicates and gaps; at_limits: every partition begins at the type's minimum and ends at its maximum"""
    info = np.iinfo(dtype)
    rows = len(part)
    out = np.empty(rows, dtype=dtype)
    heads = np.flatnonzero(part).tolist() + [rows]
    for a, z in zip(heads[:-1], heads[1:]):
        steps = rng.choice(np.array(step_choices, dtype=np.int64), size=z - a)
        steps[0] = 0
        v = np.cumsum(steps)
        span = int(info.max) - int(info.min)
        if int(v[-1]) > span:
            v = v % (span + 1)
            v.sort()
        vals = [int(info.min) + int(t) for t in v]
        if at_limits and z - a >= 2:
            half = (z - a) // 2
            vals = vals[:half] + [int(info.max) - (int(v[-1]) - int(t)) for t in v[half:]]
        if descending:
            vals = vals[::-1]
        out[a:z] = np.array(vals, dtype=object).astype(dtype)
    return out
