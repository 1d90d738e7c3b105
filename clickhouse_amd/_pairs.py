"""What the operators that keep (group key, value) pairs in HBM beside an Aggregator share over the C ABI (uniq.py, quantile.py): the
dtype tags, the handle's lifetime, add_block, merge, len and the export of the pairs.  A subclass names its C functions' prefix."""
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


class PairOperator:
    _prefix = None   # "chgpu_uniq": the operator's functions are chgpu_uniq_create, chgpu_uniq_add_block, ...

    def __init__(self, key_dtype, value_dtype, ctx: Context | None, *create_args):
        self.key_tag = -1 if key_dtype is None else _tag(key_dtype, "key")
        self.value_tag = _tag(value_dtype, "value")
        self.ctx = ctx if ctx is not None else Context(0)
        h = C.c_void_p()
        K.check(self._fn("create")(self.ctx._h, self.key_tag, self.value_tag, *create_args, C.byref(h)))
        self._h = h

    def _fn(self, name):
        return getattr(K.lib(), f"{self._prefix}_{name}")

    def close(self):
        if getattr(self, "_h", None):
            self._fn("free")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_block(self, keys, values, row_begin: int = 0, row_end: int | None = None, filter=None):
        kcol = self.ctx.column(keys) if (keys is not None and self.key_tag >= 0) else None
        vcol = self.ctx.column(values)
        fcol = self.ctx.column(filter) if filter is not None else None
        row_end = vcol.size() if row_end is None else row_end
        K.check(self._fn("add_block")(self._h, kcol._h if kcol is not None else None, vcol._h, row_begin, row_end,
                                      fcol._h if fcol is not None else None))

    def merge(self, other):
        K.check(self._fn("merge")(self._h, other._h))

    def __len__(self):
        n = C.c_uint64(0)
        K.check(self._fn("size")(self._h, C.byref(n)))
        return int(n.value)

    def _export_columns(self):
        kh, vh = C.c_void_p(), C.c_void_p()
        n = C.c_uint64(0)
        K.check(self._fn("export_pairs")(self._h, C.byref(kh), C.byref(vh), C.byref(n)))
        return (Column(self.ctx, kh) if kh.value else None), Column(self.ctx, vh)

    def export_pairs(self):
        """-> (keys ndarray or None, values ndarray)"""
        k, v = self._export_columns()
        return (k.numpy() if k is not None else None), v.numpy()
