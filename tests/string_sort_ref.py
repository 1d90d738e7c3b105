"""TEST INFRASTRUCTURE ONLY -- the reference for ColumnString::getPermutation(direction, Stable, limit) without collation and for
ColumnString::permute, over Python `bytes`, next to string_ref.py.

The order is that of `bytes`: unsigned bytes over the common length, then the shorter value is the smaller one.  `sorted` is stable and,
with reverse=True, keeps equal elements in their incoming order too, so the permutation is unique in both directions.

word_round_model restates the scheme the kernels implement (an MSD sort in 8-byte words with the key (word, c), segments that carry
their own depth and skip what all their rows share) as plain Python, so that the scheme itself is pinned against `sorted` without a GPU.
"""
from __future__ import annotations

import numpy as np

from oracle.sorting import sort_block as _oracle_sort_block


def get_permutation(values, descending=False, perm_in=None, limit=0):
    """rows (perm_in order, or row order) sorted stably by their value; entries of perm_in >= len(values) count as row 0"""
    n = len(values)
    rows = list(range(n)) if perm_in is None else [int(r) if int(r) < n else 0 for r in perm_in]
    out = sorted(rows, key=lambda i: values[i], reverse=bool(descending))
    return out[:limit] if limit and limit < len(out) else out


def sort_block(description):
    """description: [(column, descending, nan_direction_hint), ...] most significant first; a column is a numeric ndarray or a list of
    bytes.  The lexicographic comparator of oracle/sorting.py (ties by row number) -> permutation as a list"""
    cols = []
    for c, desc, hint in description:
        if not isinstance(c, np.ndarray):
            a = np.empty(len(c), dtype=object)
            a[:] = list(c)
            c = a
        cols.append((c, desc, hint))
    return [int(r) for r in _oracle_sort_block(cols)]


def key_at(value: bytes, depth: int, descending: bool):
    """(word, c) of a value at word depth `depth`"""
    rest = value[8 * depth:8 * depth + 8]
    word = int.from_bytes(rest.ljust(8, b"\0"), "big")
    c = min(9, max(0, len(value) - 8 * depth))
    return ((~word) & (2**64 - 1), 9 - c) if descending else (word, c)


def _shared_words(a: bytes, b: bytes, depth: int) -> int:
    words = min(len(a), len(b)) // 8
    k = 0
    while depth + k < words and a[8 * (depth + k):8 * (depth + k) + 8] == b[8 * (depth + k):8 * (depth + k) + 8]:
        k += 1
    return k


def word_round_model(values, descending=False, perm_in=None, limit=0, stats=None):
    """the kernels' scheme on the host -> permutation; stats (a list) receives the active rows of every round"""
    n_rows = len(values)
    rows = list(range(n_rows)) if perm_in is None else [int(r) if int(r) < n_rows else 0 for r in perm_in]
    n = len(rows)
    lim = limit if limit and limit < n else None
    cont = 0 if descending else 9
    out = [None] * n
    segments = [(0, 0, rows)] if n else []  # (start in the output, depth, rows in incoming order)
    while segments:
        if stats is not None:
            stats.append(sum(len(s[2]) for s in segments))
        nxt = []
        for start, depth, seg_rows in segments:
            if len(seg_rows) > 1:
                depth += min(_shared_words(values[a], values[b], depth) for a, b in zip(seg_rows, seg_rows[1:]))
            keyed = sorted(seg_rows, key=lambda r: key_at(values[r], depth, descending))  # stable
            i = 0
            while i < len(keyed):
                k = key_at(values[keyed[i]], depth, descending)
                j = i
                while j < len(keyed) and key_at(values[keyed[j]], depth, descending) == k:
                    out[start + j] = keyed[j]
                    j += 1
                if k[1] == cont and j - i > 1 and (lim is None or start + i < lim):
                    nxt.append((start + i, depth + 1, keyed[i:j]))
                i = j
        segments = nxt
    return out[:lim] if lim is not None else out
