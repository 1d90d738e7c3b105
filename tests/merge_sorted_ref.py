"""TEST INFRASTRUCTURE ONLY — the stable merge of sorted runs (MergingSortedAlgorithm over SortCursor) restated twice on the CPU.

merge_cursors   the per-row form: a heap of cursors, one per run, compared column by column with compareAt semantics (NaN against a number
                answers from nan_direction_hint, NaN with NaN and -0.0 with +0.0 are equal, the result negated for descending), ties by
                the run number -- SortCursor::greaterAt's `order`.
merge_lexsort   the vectorised form: a stable np.lexsort of the concatenation over normalised keys.  For runs that are sorted the two are
                the same permutation, and both are oracle.sorting.sort_block of the concatenation.
is_sorted_ref   isAlreadySorted per run: the lowest row that orders strictly before its predecessor inside one run, or None.

A description here is [(column ndarray over the concatenation, descending, nan_direction_hint), ...], most significant first.
"""
from __future__ import annotations

import heapq
import math

import numpy as np

DTYPES = (np.int64, np.uint64, np.int32, np.uint32, np.int16, np.uint16, np.int8, np.uint8, np.float64, np.float32)


def _compare(a, b, hint):
    an = isinstance(a, float) and math.isnan(a)
    bn = isinstance(b, float) and math.isnan(b)
    if an and bn:
        return 0
    if an:
        return hint
    if bn:
        return -hint
    return (a > b) - (a < b)


def compare_rows(cols, i, j):
    """cols: [(python list, direction +1 / -1, hint)] -> -1 / 0 / 1 for row i against row j"""
    for vals, direction, hint in cols:
        r = _compare(vals[i], vals[j], hint) * direction
        if r:
            return r
    return 0


def _as_lists(description):
    return [(np.asarray(c).tolist(), -1 if desc else 1, hint) for c, desc, hint in description]


class _Cursor:
    __slots__ = ("cols", "row", "end", "order")

    def __init__(self, cols, row, end, order):
        self.cols, self.row, self.end, self.order = cols, row, end, order

    def __lt__(self, other):
        r = compare_rows(self.cols, self.row, other.row)
        return r < 0 if r else self.order < other.order


def merge_cursors(description, run_offsets, limit=0) -> np.ndarray:
    cols = _as_lists(description)
    heap = [_Cursor(cols, int(run_offsets[r]), int(run_offsets[r + 1]), r) for r in range(len(run_offsets) - 1) if run_offsets[r] < run_offsets[r + 1]]
    heapq.heapify(heap)
    total = int(run_offsets[-1])
    want = min(limit, total) if limit else total
    out = []
    while heap and len(out) < want:
        c = heap[0]
        out.append(c.row)
        c.row += 1
        if c.row < c.end:
            heapq.heapreplace(heap, c)
        else:
            heapq.heappop(heap)
    return np.array(out, dtype=np.uint64)


def normalised_keys(col, descending, hint):
    """arrays whose lexicographic order (first array most significant) is the column's order under (descending, hint)"""
    col = np.asarray(col)
    if col.dtype.kind == "f":
        nan = np.isnan(col)
        flag = np.where(nan, 1 if hint > 0 else -1, 0).astype(np.int8)
        val = np.where(nan, 0.0, col).astype(np.float64)   # the widening is exact; -0.0 == 0.0 in every comparison of the sort
        return [-flag, -val] if descending else [flag, val]
    return [~col] if descending else [col]


def merge_lexsort(description, limit=0) -> np.ndarray:
    keys = []
    for col, desc, hint in description:
        keys.extend(normalised_keys(col, desc, hint))
    n = len(description[0][0])
    perm = np.lexsort(keys[::-1]).astype(np.uint64) if n else np.zeros(0, dtype=np.uint64)   # lexsort: stable, last key most significant
    return perm[:limit] if limit else perm


def is_sorted_ref(description, run_offsets):
    cols = _as_lists(description)
    starts = set(int(x) for x in run_offsets)
    for i in range(1, int(run_offsets[-1])):
        if i not in starts and compare_rows(cols, i, i - 1) < 0:
            return i
    return None


def sort_runs(columns, spec, run_offsets):
    """columns: ndarrays over the concatenation; spec: [(position, descending, hint)].  -> the columns with every run sorted by the
    description (stable, by the vectorised form)"""
    out = [np.array(c, copy=True) for c in columns]
    for r in range(len(run_offsets) - 1):
        a, b = int(run_offsets[r]), int(run_offsets[r + 1])
        perm = merge_lexsort([(columns[pos][a:b], desc, hint) for pos, desc, hint in spec]).astype(np.int64)
        for k, c in enumerate(columns):
            out[k][a:b] = c[a:b][perm]
    return out


def describe(columns, spec):
    return [(columns[pos], desc, hint) for pos, desc, hint in spec]


def offsets_of(run_lens):
    return np.concatenate([[0], np.cumsum(np.asarray(run_lens, dtype=np.int64))]).astype(np.uint64)


def random_column(rng, dtype, n, distinct=7):
    """few distinct values, so that ties are the rule; floats carry NaN, -0.0, +0.0 and the infinities"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        pool = np.array([np.nan, -0.0, 0.0, -np.inf, np.inf, 1.5, -2.25, 3.0e10, -1.0e-30], dtype=dtype)
        return pool[rng.integers(0, len(pool), size=n)]
    info = np.iinfo(dtype)
    pool = np.concatenate([np.array([info.min, info.max, 0], dtype=dtype), rng.integers(info.min, info.max, size=distinct, dtype=dtype, endpoint=True)])
    return pool[rng.integers(0, len(pool), size=n)]
