"""uniqExact(x) / count(DISTINCT x) under GROUP BY over the C ABI (AggregateFunctionUniqExact: a HashSet<T> per group): one instance ==
one exact set of (group key, value) pairs living in HBM, beside the Aggregator that holds the GROUP BY's other aggregates.
add_block / merge / export_pairs / finalize follow executeOnBlock / merge / convertToBlock not-final / final."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from ._pairs import PairOperator
from .columns import Column, Context


class UniqExact(PairOperator):
    _prefix = "chgpu_uniq"

    def __init__(self, key_dtype, value_dtype, ctx: Context | None = None, size_hint: int = 0):
        """key_dtype: an integer dtype, None = without key.  value_dtype: any column dtype; two values are equal when their bits are
        (+0.0 and -0.0 differ, NaNs with one payload are one value).  size_hint: distinct pairs expected, 0 = unknown."""
        super().__init__(key_dtype, value_dtype, ctx, int(size_hint))

    def add_block(self, keys, values, row_begin: int = 0, row_end: int | None = None, filter=None):
        """rows [row_begin, row_end) whose filter byte is non-zero enter the set.  filter: WHERE, the -If condition and the negated
        null map and-ed into one UInt8 array / Column (None: every row).  keys is ignored without key (pass None)."""
        super().add_block(keys, values, row_begin, row_end, filter)

    def merge(self, other: "UniqExact"):
        """set union; other stays valid"""
        super().merge(other)

    def export_pair_columns(self):
        """-> (keys Column or None, values Column) resident in HBM: every distinct pair once, order unspecified"""
        return self._export_columns()

    def finalize_columns(self):
        """-> (keys Column or None, counts Column of UInt64) resident in HBM"""
        kh, ch = C.c_void_p(), C.c_void_p()
        n = C.c_uint64(0)
        K.check(K.lib().chgpu_uniq_finalize(self._h, C.byref(kh), C.byref(ch), C.byref(n)))
        return (Column(self.ctx, kh) if kh.value else None), Column(self.ctx, ch)

    def finalize(self):
        """-> (keys ndarray or None, counts ndarray of uint64): one row per key that has a pair, order unspecified; without key one row"""
        k, c = self.finalize_columns()
        return (k.numpy() if k is not None else None), c.numpy()

    def counts_for_keys_column(self, keys) -> Column:
        ch = C.c_void_p()
        kcol = self.ctx.column(keys)   # (held until the call returns)
        K.check(K.lib().chgpu_uniq_counts_for_keys(self._h, kcol._h, C.byref(ch)))
        return Column(self.ctx, ch)

    def counts_for_keys(self, keys) -> np.ndarray:
        """every row's key -> that key's distinct count, 0 for a key the set lacks: the uniqExact column beside an Aggregator's
        finalize, in its row order"""
        return self.counts_for_keys_column(keys).numpy()
