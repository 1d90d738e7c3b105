"""quantileExact / quantilesExact / medianExact (and the Low / High forms) under GROUP BY over the C ABI (AggregateFunctionQuantile over
QuantileExact: an array of the values per group, selected at the end): one instance == the multiset of (group key, value) pairs living
in HBM, beside the Aggregator that holds the GROUP BY's other aggregates.  add_block / merge / export_pairs / finalize follow
executeOnBlock / merge / convertToBlock not-final / final; levels and kind belong to finalize, so one state serves any of them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from ._pairs import PairOperator
from .columns import Column, Context

KINDS = {"exact": K.QUANTILE_EXACT, "low": K.QUANTILE_EXACT_LOW, "high": K.QUANTILE_EXACT_HIGH,
         # reserved: the library answers NOT_IMPLEMENTED
         "inclusive": K.QUANTILE_EXACT_INCLUSIVE, "exclusive": K.QUANTILE_EXACT_EXCLUSIVE, "weighted": K.QUANTILE_EXACT_WEIGHTED}


def _kind(kind):
    if isinstance(kind, str):
        try:
            return KINDS[kind]
        except KeyError:
            raise ValueError(f"kind {kind!r} is not one of {sorted(KINDS)}") from None
    return int(kind)


def _levels(levels):
    a = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    return len(a), (C.c_double * max(len(a), 1))(*a.tolist())


class QuantileExact(PairOperator):
    _prefix = "chgpu_quantile"

    def __init__(self, key_dtype, value_dtype, ctx: Context | None = None):
        """key_dtype: an integer dtype, None = without key.  value_dtype: any column dtype.  A NaN value never enters; the answer for a
        level is one of the group's elements, bit for bit."""
        super().__init__(key_dtype, value_dtype, ctx)

    def add_block(self, keys, values, row_begin: int = 0, row_end: int | None = None, filter=None):
        """rows [row_begin, row_end) whose filter byte is non-zero and whose value is not NaN enter.  filter: WHERE, the -If condition
        and the negated null map and-ed into one UInt8 array / Column (None: every row).  keys is ignored without key (pass None)."""
        super().add_block(keys, values, row_begin, row_end, filter)

    def merge(self, other: "QuantileExact"):
        """multiset union; other stays valid"""
        super().merge(other)

    def export_pairs_columns(self):
        """-> (keys Column or None, values Column) resident in HBM: every held value with its key, order unspecified"""
        return self._export_columns()

    def finalize_columns(self, levels, kind="exact"):
        """-> (keys Column or None, [one Column of the value type per level]) resident in HBM"""
        n, arr = _levels(levels)
        kh = C.c_void_p()
        res = (C.c_void_p * max(n, 1))()
        groups = C.c_uint64(0)
        K.check(K.lib().chgpu_quantile_finalize(self._h, _kind(kind), n, arr, C.byref(kh), res, C.byref(groups)))
        return (Column(self.ctx, kh) if kh.value else None), [Column(self.ctx, C.c_void_p(res[i])) for i in range(n)]

    def finalize(self, levels, kind="exact"):
        """-> (keys ndarray or None, [ndarray per level]): one row per key that holds a value, order unspecified; without key one row"""
        k, cols = self.finalize_columns(levels, kind)
        return (k.numpy() if k is not None else None), [c.numpy() for c in cols]

    def quantiles_for_keys_column(self, keys, levels, kind="exact"):
        n, arr = _levels(levels)
        res = (C.c_void_p * max(n, 1))()
        kcol = self.ctx.column(keys)   # (held until the call returns)
        K.check(K.lib().chgpu_quantile_for_keys(self._h, _kind(kind), n, arr, kcol._h, res))
        return [Column(self.ctx, C.c_void_p(res[i])) for i in range(n)]

    def quantiles_for_keys(self, keys, levels, kind="exact"):
        """every row's key -> that key's quantiles, one ndarray per level; the empty-state value (NaN / 0) for a key the operator
        lacks: the quantile columns beside an Aggregator's finalize, in its row order"""
        return [c.numpy() for c in self.quantiles_for_keys_column(keys, levels, kind)]
