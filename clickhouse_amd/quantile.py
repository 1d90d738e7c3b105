"""quantileExact / quantilesExact / medianExact (and the Low / High forms) under GROUP BY over the C ABI (AggregateFunctionQuantile over
QuantileExact: an array of the values per group, selected at the end): one instance == the multiset of (group key, value) pairs living
in HBM, beside the Aggregator that holds the GROUP BY's other aggregates.  add_block / merge / export_pairs / finalize follow
executeOnBlock / merge / convertToBlock not-final / final; levels and kind belong to finalize, so one state serves any of them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from .columns import TAG_OF, Column, Context

KINDS = {"exact": K.QUANTILE_EXACT, "low": K.QUANTILE_EXACT_LOW, "high": K.QUANTILE_EXACT_HIGH,
         # reserved: the library answers NOT_IMPLEMENTED
         "inclusive": K.QUANTILE_EXACT_INCLUSIVE, "exclusive": K.QUANTILE_EXACT_EXCLUSIVE, "weighted": K.QUANTILE_EXACT_WEIGHTED}


def _tag(dtype, what):
    try:
        return TAG_OF[np.dtype(dtype)]
    except (KeyError, TypeError):
        raise ValueError(f"{what} dtype {dtype!r} is not one of the column types") from None


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


class QuantileExact:
    def __init__(self, key_dtype, value_dtype, ctx: Context | None = None):
        """key_dtype: an integer dtype, None = without key.  value_dtype: any column dtype.  A NaN value never enters; the answer for a
        level is one of the group's elements, bit for bit."""
        self.key_tag = -1 if key_dtype is None else _tag(key_dtype, "key")
        self.value_tag = _tag(value_dtype, "value")
        self.ctx = ctx if ctx is not None else Context(0)
        h = C.c_void_p()
        K.check(K.lib().chgpu_quantile_create(self.ctx._h, self.key_tag, self.value_tag, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            K.lib().chgpu_quantile_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_block(self, keys, values, row_begin: int = 0, row_end: int | None = None, filter=None):
        """rows [row_begin, row_end) whose filter byte is non-zero and whose value is not NaN enter.  filter: WHERE, the -If condition
        and the negated null map and-ed into one UInt8 array / Column (None: every row).  keys is ignored without key (pass None)."""
        kcol = self.ctx.column(keys) if (keys is not None and self.key_tag >= 0) else None
        vcol = self.ctx.column(values)
        fcol = self.ctx.column(filter) if filter is not None else None
        row_end = vcol.size() if row_end is None else row_end
        K.check(K.lib().chgpu_quantile_add_block(self._h, kcol._h if kcol is not None else None, vcol._h, row_begin, row_end,
                                                 fcol._h if fcol is not None else None))

    def merge(self, other: "QuantileExact"):
        """multiset union; other stays valid"""
        K.check(K.lib().chgpu_quantile_merge(self._h, other._h))

    def __len__(self):
        n = C.c_uint64(0)
        K.check(K.lib().chgpu_quantile_size(self._h, C.byref(n)))
        return int(n.value)

    def export_pairs_columns(self):
        """-> (keys Column or None, values Column) resident in HBM: every held value with its key, order unspecified"""
        kh, vh = C.c_void_p(), C.c_void_p()
        n = C.c_uint64(0)
        K.check(K.lib().chgpu_quantile_export_pairs(self._h, C.byref(kh), C.byref(vh), C.byref(n)))
        return (Column(self.ctx, kh) if kh.value else None), Column(self.ctx, vh)

    def export_pairs(self):
        """-> (keys ndarray or None, values ndarray)"""
        k, v = self.export_pairs_columns()
        return (k.numpy() if k is not None else None), v.numpy()

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
