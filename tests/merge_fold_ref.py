"""TEST INFRASTRUCTURE ONLY — the folding merges of MergeTree (ReplacingSortedAlgorithm, CollapsingSortedAlgorithm, SummingSortedAlgorithm,
AggregatingSortedAlgorithm over SimpleAggregateFunction columns) restated twice on the CPU, as include/chgpu.h states them.

*_cursor   the per-row form: rows arrive in merged order (merge_sorted_ref.merge_cursors), a group ends where the row differs from its
           predecessor on a key column (compare_rows == 0 is hasEqualSortColumnsWith), and the state is updated row by row the way the
           reference's loop does it.
*_vector   the vectorised form: merge_sorted_ref.merge_lexsort for the order, group starts from the normalised keys, np.*.reduceat over
           the starts.

A description is merge_sorted_ref's: [(column ndarray over the concatenation, descending, nan_direction_hint), ...].  Row numbers are
concatenated row numbers, UInt64.  A sign / is_deleted value outside its domain raises BadValue(row) for the LOWEST such row.
"""
from __future__ import annotations

import numpy as np

from merge_sorted_ref import _as_lists, compare_rows, merge_cursors, merge_lexsort, normalised_keys

U64 = np.uint64


class BadValue(ValueError):
    def __init__(self, what, row):
        super().__init__(f"{what} of row {row}")
        self.row = int(row)


def check_sign(sign):
    bad = np.flatnonzero((np.asarray(sign) != 1) & (np.asarray(sign) != -1))
    if len(bad):
        raise BadValue("sign", bad[0])


def check_is_deleted(is_deleted):
    bad = np.flatnonzero(np.asarray(is_deleted) > 1)
    if len(bad):
        raise BadValue("is_deleted", bad[0])


def _rows(xs):
    return np.array(xs, dtype=U64)


# ---------------------------------------------------------------------------------------------
# the per-row forms
# ---------------------------------------------------------------------------------------------
def _merged_groups(description, run_offsets):
    """yields (row, starts_a_group) in merged order"""
    cols = _as_lists(description)
    prev = None
    for row in merge_cursors(description, run_offsets).tolist():
        yield row, prev is None or compare_rows(cols, row, prev) != 0
        prev = row


def replacing_cursor(description, run_offsets, version=None, is_deleted=None, cleanup=False):
    if is_deleted is not None:
        check_is_deleted(is_deleted)
    ver = None if version is None else np.asarray(version).tolist()
    out, selected = [], None

    def insert_row():
        if not (cleanup and is_deleted is not None and is_deleted[selected] == 1):
            out.append(selected)

    for row, head in _merged_groups(description, run_offsets):
        if head and selected is not None:
            insert_row()
            selected = None
        if ver is None or selected is None or ver[row] >= ver[selected]:   # compareAt(..) >= 0: the later row wins a tie
            selected = row
    if selected is not None:
        insert_row()
    return _rows(out)


def collapsing_cursor(description, run_offsets, sign):
    check_sign(sign)
    sg = np.asarray(sign).tolist()
    out = []
    st = dict(cp=0, cn=0, first_negative=None, last_positive=None, last_is_positive=False)

    def insert_rows():
        if st["cp"] == 0 and st["cn"] == 0:
            return
        if st["last_is_positive"] or st["cp"] != st["cn"]:
            if st["cp"] <= st["cn"]:
                out.append(st["first_negative"])
            if st["cp"] >= st["cn"]:
                out.append(st["last_positive"])

    for row, head in _merged_groups(description, run_offsets):
        if head:
            insert_rows()
            st.update(cp=0, cn=0, first_negative=None, last_positive=None, last_is_positive=False)
        if sg[row] == 1:
            st["cp"] += 1
            st["last_is_positive"] = True
            st["last_positive"] = row
        else:
            if not st["cn"]:
                st["first_negative"] = row
            st["cn"] += 1
            st["last_is_positive"] = False
    insert_rows()
    return _rows(out)


def folding_cursor(description, run_offsets, values, kinds, drop_zero=False):
    """-> (first_rows, last_rows, [result array per value])"""
    values = [np.asarray(v) for v in values]
    firsts, lasts, results = [], [], [[] for _ in values]
    state, first, last = None, None, None

    def finish():
        if values and drop_zero and all(int(s) == 0 for s, k in zip(state, kinds) if k == "sum"):
            return
        firsts.append(first)
        lasts.append(last)
        for k, s in enumerate(state):
            results[k].append(s)

    with np.errstate(over="ignore"):
        for row, head in _merged_groups(description, run_offsets):
            if head:
                if first is not None:
                    finish()
                first, state = row, [v[row] for v in values]
            else:
                for k, v in enumerate(values):
                    x = v[row]
                    if kinds[k] == "sum":
                        state[k] = v.dtype.type(state[k] + x)   # wrap-around in the column's own type
                    elif kinds[k] == "min":
                        state[k] = min(state[k], x)
                    else:
                        state[k] = max(state[k], x)
            last = row
        if first is not None:
            finish()
    return _rows(firsts), _rows(lasts), [np.array(r, dtype=v.dtype) for r, v in zip(results, values)]


# ---------------------------------------------------------------------------------------------
# the vectorised forms
# ---------------------------------------------------------------------------------------------
def merged_groups_vector(description):
    """-> (perm as int64, starts, ends): group g is the merged positions starts[g] .. ends[g]"""
    perm = merge_lexsort(description).astype(np.int64)
    n = len(perm)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return perm, z, z
    head = np.zeros(n, dtype=bool)
    head[0] = True
    for col, desc, hint in description:
        for k in normalised_keys(col, desc, hint):
            k = k[perm]
            head[1:] |= k[1:] != k[:-1]
    starts = np.flatnonzero(head)
    ends = np.concatenate([starts[1:] - 1, [n - 1]])
    return perm, starts, ends


def replacing_vector(description, version=None, is_deleted=None, cleanup=False):
    if is_deleted is not None:
        check_is_deleted(is_deleted)
    perm, starts, ends = merged_groups_vector(description)
    if len(perm) == 0:
        return _rows([])
    if version is None:
        pos = ends
    else:
        v = np.asarray(version)[perm]
        top = np.repeat(np.maximum.reduceat(v, starts), ends - starts + 1)
        pos = np.maximum.reduceat(np.where(v == top, np.arange(len(perm)), -1), starts)
    rows = perm[pos]
    if cleanup and is_deleted is not None:
        rows = rows[np.asarray(is_deleted)[rows] != 1]
    return rows.astype(U64)


def collapsing_vector(description, sign):
    check_sign(sign)
    perm, starts, ends = merged_groups_vector(description)
    n = len(perm)
    if n == 0:
        return _rows([])
    positive = np.asarray(sign)[perm] == 1
    at = np.arange(n)
    cp = np.add.reduceat(positive.astype(np.int64), starts)
    cn = np.add.reduceat((~positive).astype(np.int64), starts)
    first_negative = np.minimum.reduceat(np.where(~positive, at, n), starts)
    last_positive = np.maximum.reduceat(np.where(positive, at, -1), starts)
    keep = positive[ends] | (cp != cn)
    pair = np.stack([np.where(keep & (cp <= cn), first_negative, -1), np.where(keep & (cp >= cn), last_positive, -1)], axis=1).ravel()
    return perm[pair[pair >= 0]].astype(U64)


def folding_vector(description, values, kinds, drop_zero=False):
    values = [np.asarray(v) for v in values]
    perm, starts, ends = merged_groups_vector(description)
    if len(perm) == 0:
        return _rows([]), _rows([]), [np.zeros(0, dtype=v.dtype) for v in values]
    op = {"sum": np.add, "min": np.minimum, "max": np.maximum}
    results = [op[k].reduceat(v[perm], starts, dtype=v.dtype) for v, k in zip(values, kinds)]
    keep = np.ones(len(starts), dtype=bool)
    if values and drop_zero:
        zero = np.ones(len(starts), dtype=bool)
        for r, k in zip(results, kinds):
            if k == "sum":
                zero &= r == 0
        keep = ~zero
    return perm[starts][keep].astype(U64), perm[ends][keep].astype(U64), [r[keep] for r in results]
