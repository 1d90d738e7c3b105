"""SELECT DISTINCT and LIMIT n [OFFSET m] BY over the C ABI (DistinctTransform / LimitByTransform): one instance == a key -> counter
table living in HBM across blocks.  filter_block answers a block with an IColumn::Filter (UInt8 Column of 0 / 1) and the number of rows
that pass; distinct_block / limit_by_block build the key of a Block the way the GROUP BY classes do and filter every column by it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from ._pairs import _tag
from .columns import Column, Context, filter_columns, pack_fixed_keys
from .keysfixed import KeyDict
from .lowcardinality import ColumnLowCardinality, ColumnString, LowCardinalityDictionary


class LimitBy:
    def __init__(self, key_dtype, length: int, offset: int = 0, size_hint: int = 0, ctx: Context | None = None):
        """key_dtype: an integer dtype of 1-8 bytes (ids and packed keys are ordinary keys).  A row passes when the number of earlier
        rows of its key, over every block so far, lies in [offset, offset + length)."""
        self.key_tag = _tag(key_dtype, "key")
        if length < 0 or offset < 0 or size_hint < 0:
            raise ValueError(f"length {length!r}, offset {offset!r} and size_hint {size_hint!r} must not be negative")
        self.length, self.offset = int(length), int(offset)
        self.ctx = ctx if ctx is not None else Context(0)
        h = C.c_void_p()
        K.check(K.lib().chgpu_limit_by_create(self.ctx._h, self.key_tag, self.length, self.offset, int(size_hint), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            K.lib().chgpu_limit_by_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def filter_block(self, keys, row_begin: int = 0, row_end: int | None = None, filter=None):
        """rows [row_begin, row_end) in row order; a row whose filter byte (WHERE; None: every row) is zero gets 0 and counts nowhere.
        -> (UInt8 Column of row_end - row_begin bytes, rows that pass)"""
        kcol = self.ctx.column(keys)
        fcol = self.ctx.column(filter) if filter is not None else None
        row_end = kcol.size() if row_end is None else row_end
        out = C.c_void_p()
        passed = C.c_uint64(0)
        K.check(K.lib().chgpu_limit_by_filter_block(self._h, kcol._h, row_begin, row_end, fcol._h if fcol is not None else None, C.byref(out), C.byref(passed)))
        return Column(self.ctx, out), int(passed.value)

    def keys(self) -> int:
        """keys that have been counted at least once"""
        n = C.c_uint64(0)
        K.check(K.lib().chgpu_limit_by_keys(self._h, C.byref(n)))
        return int(n.value)


class Distinct(LimitBy):
    def __init__(self, key_dtype, size_hint: int = 0, ctx: Context | None = None):
        super().__init__(key_dtype, 1, 0, size_hint=size_hint, ctx=ctx)


class BlockKeys:
    """The state limit_by_block keeps over a query: how the key columns become one integer column (decided at the first block), the
    dictionaries that takes, and the operator over that column."""

    def __init__(self, length: int = 1, offset: int = 0, size_hint: int = 0, ctx: Context | None = None):
        self.length, self.offset, self.size_hint = length, offset, size_hint
        self.ctx = ctx if ctx is not None else Context(0)
        self.op = None
        self.lc_dicts = {}   # key position -> LowCardinalityDictionary (String / LowCardinality keys)
        self.keydict = None  # fixed-width keys of more than 8 bytes together

    def close(self):
        if self.op is not None:
            self.op.close()
        if self.keydict is not None:
            self.keydict.close()

    def _fixed(self, pos, col) -> Column:
        """a key column as a fixed-width Column: Strings and LowCardinality through a query-wide dictionary's UInt32 ids"""
        if isinstance(col, ColumnString):
            col = col.dictionary_encode()
        if isinstance(col, ColumnLowCardinality):
            dic = self.lc_dicts.setdefault(pos, LowCardinalityDictionary(self.ctx))
            return dic.map_block(col)
        return self.ctx.column(col)

    def key_column(self, key_cols) -> Column:
        """one column as is; several of <= 8 bytes together through packFixed; wider through a KeyDict's ids"""
        cols = [self._fixed(pos, c) for pos, c in enumerate(key_cols)]
        if not cols:
            raise ValueError("no key column: without a key the clause is a plain LIMIT")
        if len(cols) == 1:
            key = cols[0]
        elif sum(c.dtype.itemsize for c in cols) <= 8:
            key = pack_fixed_keys(cols)
        else:
            if self.keydict is None:
                self.keydict = KeyDict([c.dtype for c in cols], ctx=self.ctx, size_hint=self.size_hint)
            key = self.keydict.encode(cols)
        if self.op is None:
            self.op = LimitBy(key.dtype, self.length, self.offset, size_hint=self.size_hint, ctx=self.ctx)
        return key


def _filter_any(col, filt: Column):
    return col.filter(filt)


def limit_by_block(op: BlockKeys, key_cols, columns):
    """LimitByTransform::transform over one Block: key_cols are positions into `columns` (Column / ColumnString /
    ColumnLowCardinality / ndarray).  -> the surviving rows of every column; None when no row survives; `columns` itself when every
    row does."""
    key = op.key_column([columns[p] for p in key_cols])
    filt, passed = op.op.filter_block(key)
    if passed == 0:
        return None
    if passed == key.size():
        return columns
    plain = [k for k, c in enumerate(columns) if not isinstance(c, (ColumnString, ColumnLowCardinality))]
    done = dict(zip(plain, filter_columns([op.ctx.column(columns[k]) for k in plain], filt, passed))) if plain else {}
    return [done[k] if k in done else _filter_any(c, filt) for k, c in enumerate(columns)]


def distinct_block(op: BlockKeys, columns):
    """DistinctTransform::transform over one Block: every column is a key"""
    return limit_by_block(op, list(range(len(columns))), columns)
