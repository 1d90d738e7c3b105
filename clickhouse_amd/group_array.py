"""groupArray(x) / groupArray(N)(x) under GROUP BY over the C ABI (AggregateFunctionGroupArray: an array of the values per group, in
arrival order): one instance == the (group key, value) pairs living in HBM in the order they entered, beside the Aggregator that holds
the GROUP BY's other aggregates.  add_block / merge / export_pairs / finalize follow executeOnBlock / merge / convertToBlock not-final /
final; the result is a ColumnArray in two columns: offsets[i] is where array i ends, data holds the arrays one after another."""
from __future__ import annotations

import ctypes as C

from . import _capi as K
from ._pairs import PairOperator
from .columns import Column, Context


class GroupArray(PairOperator):
    _prefix = "chgpu_group_array"

    def __init__(self, key_dtype, value_dtype, max_size: int = 0, ctx: Context | None = None):
        """key_dtype: an integer dtype, None = without key.  value_dtype: any column dtype; every value comes back bit for bit, NaNs
        included.  max_size: N of groupArray(N), 0 = no limit."""
        if max_size < 0:
            raise ValueError(f"max_size {max_size!r} is negative")
        self.max_size = int(max_size)
        super().__init__(key_dtype, value_dtype, ctx, C.c_uint64(self.max_size))

    def add_block(self, keys, values, row_begin: int = 0, row_end: int | None = None, filter=None):
        """rows [row_begin, row_end) whose filter byte is non-zero enter, in row order, behind everything that entered before.  filter:
        WHERE, the -If condition and the negated null map and-ed into one UInt8 array / Column (None: every row).  keys is ignored
        without key (pass None)."""
        super().add_block(keys, values, row_begin, row_end, filter)

    def merge(self, other: "GroupArray"):
        """other's values behind this operator's, group by group; other stays valid; both of one max_size"""
        super().merge(other)

    def export_pairs_columns(self):
        """-> (keys Column or None, values Column) resident in HBM: every held pair in store order"""
        return self._export_columns()

    def finalize_columns(self):
        """-> (keys Column or None, offsets Column (UInt64), data Column of the value type) resident in HBM"""
        kh, oh, dh = C.c_void_p(), C.c_void_p(), C.c_void_p()
        groups = C.c_uint64(0)
        K.check(K.lib().chgpu_group_array_finalize(self._h, C.byref(kh), C.byref(oh), C.byref(dh), C.byref(groups)))
        return (Column(self.ctx, kh) if kh.value else None), Column(self.ctx, oh), Column(self.ctx, dh)

    def finalize(self):
        """-> (keys ndarray or None, offsets, data): one row per key that holds a value; array i is data[offsets[i - 1]:offsets[i]].
        Without key one row, which may be the empty array."""
        k, o, d = self.finalize_columns()
        return (k.numpy() if k is not None else None), o.numpy(), d.numpy()

    def arrays_for_keys_column(self, keys):
        oh, dh = C.c_void_p(), C.c_void_p()
        kcol = self.ctx.column(keys)   # (held until the call returns)
        K.check(K.lib().chgpu_group_array_for_keys(self._h, kcol._h, C.byref(oh), C.byref(dh)))
        return Column(self.ctx, oh), Column(self.ctx, dh)

    def arrays_for_keys(self, keys):
        """every row's key -> that key's array, as (offsets, data); the empty array for a key the operator lacks: the groupArray column
        beside an Aggregator's finalize, in its row order"""
        o, d = self.arrays_for_keys_column(keys)
        return o.numpy(), d.numpy()
