"""Reference for the window operator (chgpu_window_*): WindowTransform's partitions, peer groups, frames and functions restated per row.

window_slow is the definition: plain loops over Python integers (nothing can wrap), the frame of each row taken as a slice.  window_fast
is the same in vectorised numpy for inputs too large for the loops; tests/test_window_ref.py holds the two against each other and pins
window_slow with hand-written columns.

A frame is the tuple (type, begin_kind, begin_offset, end_kind, end_offset), None is the default RANGE UNBOUNDED PRECEDING .. CURRENT ROW.
Keys and arguments are numpy arrays of the ten column dtypes; `default` of lag / lead is a value of the argument's dtype."""
import numpy as np

(ROW_NUMBER, RANK, DENSE_RANK, COUNT, SUM, AVG, MIN, MAX, FIRST_VALUE, LAST_VALUE, LAG_IN_FRAME, LEAD_IN_FRAME) = range(12)
ROWS, RANGE = 0, 1
UNBOUNDED_PRECEDING, OFFSET_PRECEDING, CURRENT_ROW, OFFSET_FOLLOWING, UNBOUNDED_FOLLOWING = range(5)
DEFAULT_FRAME = (RANGE, UNBOUNDED_PRECEDING, 0, CURRENT_ROW, 0)
U64_MAX = 2**64 - 1
FUNCTIONS_WITHOUT_ARG = (ROW_NUMBER, RANK, DENSE_RANK, COUNT)


def frame_is_legal(frame):
    """WindowFrame::checkValid"""
    _, b, bo, e, eo = frame
    if b == UNBOUNDED_FOLLOWING or e == UNBOUNDED_PRECEDING:
        return False
    if b == CURRENT_ROW and e == OFFSET_PRECEDING:
        return False
    if b == OFFSET_FOLLOWING and e in (CURRENT_ROW, OFFSET_PRECEDING):
        return False
    if b == e == OFFSET_PRECEDING and bo < eo:
        return False
    if b == e == OFFSET_FOLLOWING and bo > eo:
        return False
    return True


def frame_is_served(frame):
    """legal and not RANGE with an offset"""
    t, b, _, e, _ = frame
    return frame_is_legal(frame) and not (t == RANGE and (b in (OFFSET_PRECEDING, OFFSET_FOLLOWING) or e in (OFFSET_PRECEDING, OFFSET_FOLLOWING)))


def sum_result_dtype(dtype):
    return np.dtype(np.int64) if np.dtype(dtype).kind == "i" else np.dtype(np.uint64)


def result_dtype(function, dtype=None):
    if function in FUNCTIONS_WITHOUT_ARG:
        return np.dtype(np.uint64)
    if function == SUM:
        return sum_result_dtype(dtype)
    if function == AVG:
        return np.dtype(np.float64)
    return np.dtype(dtype)


def _equal(a, b):
    """compareAt == 0: integers by value, floats a == b or both NaN"""
    return bool(a == b) or bool(a != a and b != b)


def heads_slow(partition_cols, order_cols, rows):
    part, peer = [], []
    for i in range(rows):
        p = i == 0 or any(not _equal(c[i], c[i - 1]) for c in partition_cols)
        g = p or any(not _equal(c[i], c[i - 1]) for c in order_cols)
        part.append(p)
        peer.append(g)
    return part, peer


def bounds_slow(heads, rows):
    """first row and one past the last row of every row's run"""
    start, end = [0] * rows, [rows] * rows
    for i in range(rows):
        start[i] = i if heads[i] else start[i - 1]
    for i in range(rows - 1, -1, -1):
        end[i] = rows if i == rows - 1 else (i + 1 if heads[i + 1] else end[i + 1])
    return start, end


def frame_slow(frame, i, ps, pe, gs, ge):
    t, b, bo, e, eo = frame
    fs = {UNBOUNDED_PRECEDING: ps, OFFSET_PRECEDING: max(ps, i - bo), CURRENT_ROW: i if t == ROWS else gs, OFFSET_FOLLOWING: min(pe, i + bo)}[b]
    fe = {OFFSET_PRECEDING: max(ps, i - eo + 1), CURRENT_ROW: i + 1 if t == ROWS else ge, OFFSET_FOLLOWING: min(pe, i + eo + 1), UNBOUNDED_FOLLOWING: pe}[e]
    return fs, fe


def _bits(v):
    """the element's bits as an unsigned integer of its width"""
    return int(np.array([v]).view(f"u{np.dtype(type(v)).itemsize}")[0])


def order_key(v):
    """min / max order: integers by value; floats in IEEE total order (-NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN)"""
    dt = np.dtype(type(v))
    if dt.kind != "f":
        return int(v)
    b, w = _bits(v), 8 * dt.itemsize
    return (~b) & ((1 << w) - 1) if b >> (w - 1) else b | (1 << (w - 1))


def _wrap(total, dtype):
    total &= U64_MAX
    if np.dtype(dtype).kind == "i" and total >= 2**63:
        total -= 2**64
    return total


def window_slow(function, partition_cols, order_cols, rows, frame=None, x=None, offset=1, default=0):
    frame = DEFAULT_FRAME if frame is None else frame
    assert frame_is_served(frame) or function in (ROW_NUMBER, RANK, DENSE_RANK)
    part, peer = heads_slow(partition_cols, order_cols, rows)
    ps, pe = bounds_slow(part, rows)
    gs, ge = bounds_slow(peer, rows)
    dt = None if x is None else x.dtype
    out = np.zeros(rows, dtype=result_dtype(function, dt))
    for i in range(rows):
        if function == ROW_NUMBER:
            out[i] = i - ps[i] + 1
            continue
        if function == RANK:
            out[i] = gs[i] - ps[i] + 1
            continue
        if function == DENSE_RANK:
            out[i] = sum(1 for j in range(ps[i], i + 1) if peer[j])
            continue
        fs, fe = frame_slow(frame, i, ps[i], pe[i], gs[i], ge[i])
        assert fs <= fe
        if function == COUNT:
            out[i] = fe - fs
            continue
        rows_of_frame = x[fs:fe]
        if function == SUM:
            out[i] = _wrap(sum(int(v) for v in rows_of_frame), dt)
        elif function == AVG:
            num = _wrap(sum(int(v) for v in rows_of_frame), dt)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[i] = np.float64(num) / np.float64(fe - fs)
        elif function in (MIN, MAX):
            if len(rows_of_frame):
                out[i] = (min if function == MIN else max)(rows_of_frame, key=order_key)
        elif function == FIRST_VALUE:
            if len(rows_of_frame):
                out[i] = rows_of_frame[0]
        elif function == LAST_VALUE:
            if len(rows_of_frame):
                out[i] = rows_of_frame[-1]
        else:
            t = i - offset if function == LAG_IN_FRAME else i + offset
            out[i] = x[t] if fs <= t < fe else default
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the same, vectorised
# ---------------------------------------------------------------------------------------------------------------------------------
def heads_fast(partition_cols, order_cols, rows):
    def differs(cols):
        d = np.zeros(rows, dtype=bool)
        for c in cols:
            a, b = c[1:], c[:-1]
            eq = a == b
            if c.dtype.kind == "f":
                eq |= np.isnan(a) & np.isnan(b)
            d[1:] |= ~eq
        return d
    part = differs(partition_cols)
    peer = part | differs(order_cols)
    if rows:
        part[0] = peer[0] = True
    return part, peer


def bounds_fast(heads, rows):
    idx = np.arange(rows, dtype=np.int64)
    start = np.maximum.accumulate(np.where(heads, idx, 0))
    nxt = np.full(rows, rows, dtype=np.int64)          # the next head after row i, or rows
    nxt[:-1] = np.where(heads[1:], idx[1:], rows)
    end = np.minimum.accumulate(nxt[::-1])[::-1]
    return start, end


def frames_fast(frame, rows, ps, pe, gs, ge):
    t, b, bo, e, eo = frame
    i = np.arange(rows, dtype=np.int64)
    bo, eo = min(bo, rows + 1), min(eo, rows + 1)      # an offset past every row acts like rows + 1: nothing wraps
    fs = {UNBOUNDED_PRECEDING: ps, OFFSET_PRECEDING: np.maximum(ps, i - bo), CURRENT_ROW: i if t == ROWS else gs, OFFSET_FOLLOWING: np.minimum(pe, i + bo)}[b]
    fe = {OFFSET_PRECEDING: np.maximum(ps, i - eo + 1), CURRENT_ROW: i + 1 if t == ROWS else ge, OFFSET_FOLLOWING: np.minimum(pe, i + eo + 1),
          UNBOUNDED_FOLLOWING: pe}[e]
    return fs, fe


def order_keys_fast(x):
    if x.dtype.kind == "i":
        return x.astype(np.int64).view(np.uint64) ^ np.uint64(2**63)
    if x.dtype.kind == "u":
        return x.astype(np.uint64)
    w = 8 * x.dtype.itemsize
    b = x.view(f"u{x.dtype.itemsize}").astype(np.uint64)
    neg = (b >> np.uint64(w - 1)) != 0
    return np.where(neg, ~b & np.uint64((1 << w) - 1), b | np.uint64(1 << (w - 1)))


def _running_extremum_rows(keys, part, is_min, backward):
    """for every row the row number of the extremum of its partition up to the row (backward: from the row on)"""
    n = len(keys)
    if backward:
        part_rev = np.zeros(n, dtype=bool)
        part_rev[0] = True
        part_rev[1:] = part[::-1][:-1]                 # in reversed order a run starts behind a head of the original order
        return n - 1 - _running_extremum_rows(keys[::-1], part_rev, is_min, False)[::-1]
    order = np.argsort(keys, kind="stable")
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n, dtype=np.int64)
    if is_min:
        rank = n - 1 - rank
    pid = np.cumsum(part).astype(np.int64)
    run = np.maximum.accumulate(pid * (n + 1) + rank) - pid * (n + 1)
    if is_min:
        run = n - 1 - run
    return order[run]


def window_fast(function, partition_cols, order_cols, rows, frame=None, x=None, offset=1, default=0):
    frame = DEFAULT_FRAME if frame is None else frame
    part, peer = heads_fast(partition_cols, order_cols, rows)
    ps, pe = bounds_fast(part, rows)
    gs, ge = bounds_fast(peer, rows)
    i = np.arange(rows, dtype=np.int64)
    dt = None if x is None else x.dtype
    rdt = result_dtype(function, dt)
    if rows == 0:
        return np.zeros(0, dtype=rdt)
    if function == ROW_NUMBER:
        return (i - ps + 1).astype(rdt)
    if function == RANK:
        return (gs - ps + 1).astype(rdt)
    if function == DENSE_RANK:
        c = np.cumsum(peer).astype(np.int64)
        return (c - c[ps] + 1).astype(rdt)
    fs, fe = frames_fast(frame, rows, ps, pe, gs, ge)
    if function == COUNT:
        return (fe - fs).astype(rdt)
    empty = fs >= fe
    if function in (SUM, AVG):
        wide = x.astype(np.int64).view(np.uint64) if dt.kind == "i" else x.astype(np.uint64)
        p = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(wide, dtype=np.uint64)])
        s = (p[fe] - p[fs]).view(sum_result_dtype(dt))
        if function == SUM:
            return s
        with np.errstate(invalid="ignore", divide="ignore"):
            return s.astype(np.float64) / (fe - fs).astype(np.float64)
    if function in (MIN, MAX):
        assert frame[1] == UNBOUNDED_PRECEDING or frame[3] == UNBOUNDED_FOLLOWING
        backward = frame[1] != UNBOUNDED_PRECEDING
        at = _running_extremum_rows(order_keys_fast(x), part, function == MIN, backward)
        src = at[np.where(empty, 0, fs if backward else fe - 1)]
    elif function == FIRST_VALUE:
        src = np.where(empty, 0, fs)
    elif function == LAST_VALUE:
        src = np.where(empty, 0, fe - 1)
    else:
        k = min(offset, rows + 1)
        t = i - k if function == LAG_IN_FRAME else i + k
        empty = ~((t >= fs) & (t < fe))
        src = np.where(empty, 0, t)
        return np.where(empty, np.array([default], dtype=dt).view(f"u{dt.itemsize}")[0], x.view(f"u{dt.itemsize}")[src]).astype(f"u{dt.itemsize}").view(dt)
    return np.where(empty, 0, x.view(f"u{dt.itemsize}")[src]).astype(f"u{dt.itemsize}").view(dt)


def same_bits(a, b):
    """bit-exact equality, except that any NaN equals any NaN in a Float64 avg column (pass nan_equal for those)"""
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}")))


def same_avg(a, b):
    """avg columns: bit-exact where a value, NaN where NaN (the sign of 0 / 0 is the divider's)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and same_bits(np.where(na, 0.0, a), np.where(nb, 0.0, b))


def frame_families(k, m):
    """one served frame of every family for the offsets k, m (ordered as each family's validity asks)"""
    lo, hi = min(k, m), max(k, m)
    return [None,
            (ROWS, UNBOUNDED_PRECEDING, 0, CURRENT_ROW, 0),
            (ROWS, UNBOUNDED_PRECEDING, 0, UNBOUNDED_FOLLOWING, 0),
            (ROWS, OFFSET_PRECEDING, k, OFFSET_FOLLOWING, m),
            (ROWS, OFFSET_PRECEDING, hi, OFFSET_PRECEDING, lo),
            (ROWS, OFFSET_FOLLOWING, lo, OFFSET_FOLLOWING, hi),
            (ROWS, CURRENT_ROW, 0, UNBOUNDED_FOLLOWING, 0),
            (RANGE, CURRENT_ROW, 0, CURRENT_ROW, 0)]


def frame_serves_extremum(frame):
    """min / max need a frame that begins UNBOUNDED PRECEDING or ends UNBOUNDED FOLLOWING"""
    frame = DEFAULT_FRAME if frame is None else frame
    return frame[1] == UNBOUNDED_PRECEDING or frame[3] == UNBOUNDED_FOLLOWING


def geometric_layout(rng, rows, mean_partition, mean_group=2.0):
    """sorted (partition key UInt32, order key Int64) columns with geometric partition and peer-group lengths"""
    part = rng.random(rows) < 1.0 / mean_partition
    peer = part | (rng.random(rows) < 1.0 / mean_group)
    if rows:
        part[0] = peer[0] = True
    p = np.cumsum(part).astype(np.uint32)
    o = np.cumsum(peer).astype(np.int64) - 7
    return p, o
