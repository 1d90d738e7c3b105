"""TEST INFRASTRUCTURE ONLY -- a vectorised restatement of the stable order of IColumn::getPermutation (oracle/sorting.py holds the
per-row comparator form, too slow past a few thousand rows).  It works on VALUES -- numpy's comparison of the column's own dtype -- never
on radix key bits, so it shares nothing with the product's key fold.

Ascending: numbers by value, ties (a == b, hence -0.0 with +0.0; NaN with NaN) by row number; every NaN after the numbers when
nan_direction_hint > 0, before them otherwise.  Descending: the ascending stable order of the REVERSED column read backwards -- values
fall, NaN lands at the other end (hint > 0: NaN is the greatest, so it leads), and a tie class, which the reversed column's stable order
lists by falling original row, comes out by rising original row again.
"""
import numpy as np


def _ascending(x, hint):
    n = x.shape[0]
    if x.dtype.kind == "f":
        nan = np.isnan(x)
        return np.lexsort((np.arange(n), np.where(nan, x.dtype.type(0), x), nan if hint > 0 else ~nan))
    return np.argsort(x, kind="stable")


def get_permutation(x, descending=False, nan_direction_hint=1):
    """-> UInt64 permutation, the same contract as oracle.sorting.get_permutation"""
    x = np.asarray(x)
    n = x.shape[0]
    if not descending:
        return _ascending(x, nan_direction_hint).astype(np.uint64)
    p = _ascending(x[::-1], nan_direction_hint)
    return (n - 1 - p[::-1]).astype(np.uint64)


def sort_block(description):
    """[(column, descending, nan_direction_hint), ...] most significant first -> UInt64 permutation: the least significant column is
    sorted first and every more significant one re-sorts that order stably (a stable sort of x[perm] composed with perm)."""
    perm = None
    for col, desc, hint in reversed(list(description)):
        col = np.asarray(col)
        if perm is None:
            perm = get_permutation(col, desc, hint)
        else:
            perm = perm[get_permutation(col[perm.astype(np.int64)], desc, hint).astype(np.int64)]
    return perm
