"""A plain ASOF join on values in their own dtype: the reference of tests/test_gpu_asof_edges.py (test_asof_ref.py holds it against
oracle.asof_pairs).  It never forms an order key, so it shares nothing with the fold of the kernels; NumPy's `<` on the column's own
dtype is the only comparison (-0.0 and +0.0 are therefore equal, and a Float32 column is never widened)."""
import numpy as np

ASOF_LESS, ASOF_GREATER, ASOF_LESS_OR_EQUALS, ASOF_GREATER_OR_EQUALS = 1, 2, 3, 4
INEQUALITIES = {"LESS": ASOF_LESS, "GREATER": ASOF_GREATER, "LESS_OR_EQUALS": ASOF_LESS_OR_EQUALS, "GREATER_OR_EQUALS": ASOF_GREATER_OR_EQUALS}
ASOF_TYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64, np.float32, np.float64]
KEY_TYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]


def _groups(keys, rows):
    """rows (indices into keys) -> {key: its rows in their given order}"""
    order = np.argsort(keys[rows], kind="stable")
    rows = rows[order]
    k = keys[rows]
    cut = np.flatnonzero(k[1:] != k[:-1]) + 1
    return {key.item(): part for key, part in zip(k[np.concatenate([[0], cut])] if rows.shape[0] else [], np.split(rows, cut))}


def asof_ref(build_blocks, left_keys, left_asof, inequality, left_null_map=None, left_join=False):
    """Same arguments and meaning as oracle.asof_pairs: build_blocks is [(keys, asof, null_map or None, join_mask or None)]; the answer is
    (left_row, block, row) as int64 arrays in left-row order, (-1, -1) being the default row of a LEFT join; an INNER join drops the left
    rows without a partner.  `block` counts every block given, empty and fully masked ones too; `row` is the position in the block as
    given.  Build rows with a NULL key, a zero ON mask or a NaN asof value are dropped; left rows with a NULL key or a NaN value have no
    partner.

    Per distinct key its rows are taken in insertion order (block, then row) and sorted stably by value; np.searchsorted then answers
    `right` - 1 for >=, `left` - 1 for >, `left` for <=, `right` for <.  Stability plus those four calls is the tie rule of the header of
    asof_kernels.hip: among build rows with equal (key, asof) the LAST inserted wins for >= and >, the FIRST inserted for <= and <."""
    ks, vs, bs, rs = [], [], [], []
    for b, (keys, asof, nm, jm) in enumerate(build_blocks):
        keep = np.ones(keys.shape[0], dtype=bool)
        if nm is not None:
            keep &= np.asarray(nm) == 0
        if jm is not None:
            keep &= np.asarray(jm) != 0
        if asof.dtype.kind == "f":
            keep &= ~np.isnan(asof)
        r = np.flatnonzero(keep)
        ks.append(keys[r])
        vs.append(asof[r])
        bs.append(np.full(r.shape[0], b, dtype=np.int64))
        rs.append(r.astype(np.int64))
    n = left_keys.shape[0]
    block = np.full(n, -1, dtype=np.int64)
    row = np.full(n, -1, dtype=np.int64)
    if ks and sum(k.shape[0] for k in ks):
        K, V, B, R = np.concatenate(ks), np.concatenate(vs), np.concatenate(bs), np.concatenate(rs)
        ok = np.ones(n, dtype=bool)
        if left_null_map is not None:
            ok &= np.asarray(left_null_map) == 0
        if left_asof.dtype.kind == "f":
            ok &= ~np.isnan(left_asof)
        right = _groups(K, np.arange(K.shape[0]))
        for key, li in _groups(left_keys, np.flatnonzero(ok)).items():
            ri = right.get(key)
            if ri is None:
                continue
            ri = ri[np.argsort(V[ri], kind="stable")]
            sv, t = V[ri], left_asof[li]
            if inequality == ASOF_GREATER_OR_EQUALS:
                p = np.searchsorted(sv, t, side="right") - 1
            elif inequality == ASOF_GREATER:
                p = np.searchsorted(sv, t, side="left") - 1
            elif inequality == ASOF_LESS_OR_EQUALS:
                p = np.searchsorted(sv, t, side="left")
            elif inequality == ASOF_LESS:
                p = np.searchsorted(sv, t, side="right")
            else:
                raise ValueError(f"inequality {inequality!r}")
            hit = (p >= 0) & (p < ri.shape[0])
            at = ri[p[hit]]
            block[li[hit]] = B[at]
            row[li[hit]] = R[at]
    left = np.arange(n, dtype=np.int64)
    if not left_join:
        m = block >= 0
        return left[m], block[m], row[m]
    return left, block, row


def value_pool(dtype, nan=True):
    """the edge values of one asof type, ascending (NaN last)"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        fi = np.finfo(dt)
        one5, two, zero = dt.type(1.5), dt.type(2.0), dt.type(0.0)
        v = [-np.inf, -fi.max, -one5, np.nextafter(-one5, zero), -fi.tiny, -fi.smallest_subnormal, -0.0, 0.0, fi.smallest_subnormal, fi.tiny,
             one5, np.nextafter(one5, two), fi.max, np.inf] + ([np.nan] if nan else [])
        return np.array(v, dtype=dt)
    ii = np.iinfo(dt)
    if ii.min < 0:
        return np.array([ii.min, ii.min + 1, -1, 0, 1, ii.max - 1, ii.max], dtype=dt)
    half = 1 << (dt.itemsize * 8 - 1)
    return np.array([0, 1, half - 1, half, ii.max - 1, ii.max], dtype=dt)


def first_difference(got, want):
    """None when the two (left_row, block, row) answers are equal, else a description of the first differing row"""
    gl, gb, gr = (np.asarray(x) for x in got)
    wl, wb, wr = (np.asarray(x) for x in want)
    n = min(gl.shape[0], wl.shape[0])
    bad = np.flatnonzero((gl[:n] != wl[:n]) | (gb[:n] != wb[:n]) | (gr[:n] != wr[:n]))
    if bad.shape[0]:
        i = int(bad[0])
        return f"output row {i}: got (left {gl[i]}, block {gb[i]}, row {gr[i]}), want (left {wl[i]}, block {wb[i]}, row {wr[i]}); {bad.shape[0]} rows differ"
    if gl.shape[0] != wl.shape[0]:
        return f"{gl.shape[0]} output rows, want {wl.shape[0]}"
    return None
