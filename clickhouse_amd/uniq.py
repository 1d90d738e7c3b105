"""uniqExact(x) / count(DISTINCT x) under GROUP BY over the C ABI (AggregateFunctionUniqExact: a HashSet<T> per group): one instance ==
one exact set of (group key, value) pairs living in HBM, beside the Aggregator that holds the GROUP BY's other aggregates.
add_block / merge / export_pairs / finalize follow executeOnBlock / merge / convertToBlock not-final / final."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from .columns import TAG_OF, Column, Context


def _tag(dtype, what):
    try:
        return TAG_OF[np.dtype(dtype)]
    except (KeyError, TypeError):
        raise ValueError(f"{what} dtype {dtype!r} is not one of the column types") from None


class UniqExact:
    def __init__(self, key_dtype, value_dtype, ctx: Context | None = None, size_hint: int = 0):
        """key_dtype: an integer dtype, None = without key.  value_dtype: any column dtype; two values are equal when their bits are
        (+0.0 and -0.0 differ, NaNs with one payload are one value).  size_hint: distinct pairs expected, 0 = unknown."""
        self.key_tag = -1 if key_dtype is None else _tag(key_dtype, "key")
        self.value_tag = _tag(value_dtype, "value")
        self.ctx = ctx if ctx is not None else Context(0)
        h = C.c_void_p()
        K.check(K.lib().chgpu_uniq_create(self.ctx._h, self.key_tag, self.value_tag, int(size_hint), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            K.lib().chgpu_uniq_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_block(self, keys, values, row_begin: int = 0, row_end: int | None = None, filter=None):
        """rows [row_begin, row_end) whose filter byte is non-zero enter the set.  filter: WHERE, the -If condition and the negated
        null map and-ed into one UInt8 array / Column (None: every row).  keys is ignored without key (pass None)."""
        kcol = self.ctx.column(keys) if (keys is not None and self.key_tag >= 0) else None
        vcol = self.ctx.column(values)
        fcol = self.ctx.column(filter) if filter is not None else None
        row_end = vcol.size() if row_end is None else row_end
        K.check(K.lib().chgpu_uniq_add_block(self._h, kcol._h if kcol is not None else None, vcol._h, row_begin, row_end,
                                             fcol._h if fcol is not None else None))

    def merge(self, other: "UniqExact"):
        """set union; other stays valid"""
        K.check(K.lib().chgpu_uniq_merge(self._h, other._h))

    def __len__(self):
        n = C.c_uint64(0)
        K.check(K.lib().chgpu_uniq_size(self._h, C.byref(n)))
        return int(n.value)

    def export_pair_columns(self):
        """-> (keys Column or None, values Column) resident in HBM: every distinct pair once, order unspecified"""
        kh, vh = C.c_void_p(), C.c_void_p()
        n = C.c_uint64(0)
        K.check(K.lib().chgpu_uniq_export_pairs(self._h, C.byref(kh), C.byref(vh), C.byref(n)))
        return (Column(self.ctx, kh) if kh.value else None), Column(self.ctx, vh)

    def export_pairs(self):
        """-> (keys ndarray or None, values ndarray)"""
        k, v = self.export_pair_columns()
        return (k.numpy() if k is not None else None), v.numpy()

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
