"""The merges of MergeTree that fold rows of equal sorting key while they merge, over the C ABI: ReplacingSortedAlgorithm,
CollapsingSortedAlgorithm, VersionedCollapsingAlgorithm, SummingSortedAlgorithm and AggregatingSortedAlgorithm over
SimpleAggregateFunction columns (src/Processors/Merges/Algorithms/).  The input is what merge_sorted takes -- sorted runs glued end to end -- and the answer is the rows
that survive, in merged order, as concatenated row numbers (and, for the folding form, one result column per folded column).  Numeric
columns only; String columns, Float value columns and bad descriptions raise before the library is touched.

The *_rows functions return the raw outputs; the Block-level functions glue the blocks, call them and index every column."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from .columns import Column, Context  # noqa: F401  (Context: the name stays patchable here, as in merge_sorted)
from .merge_sorted import _check_column, _glue_blocks, _prepare

TILE = 2048       # T: merged positions of one fold tile (FOLD_TILE of csrc/merge_fold_host.h)
MAX_VALUES = 8    # value columns of one folding call (FOLD_MAX_VALUES)
KINDS = {"sum": K.FOLD_SUM, "min": K.FOLD_MIN, "max": K.FOLD_MAX}


def _dtype_of(c):
    return c.dtype if isinstance(c, Column) else np.asarray(c).dtype


def _check_typed(c, what, kinds, expect):
    """a numeric column whose dtype kind is one of `kinds` (and, when given, exactly `expect`)"""
    _check_column(c, what)
    dt = _dtype_of(c)
    if dt.kind not in kinds or (expect is not None and dt != np.dtype(expect)):
        raise TypeError(f"{what} has dtype {dt}: it must be {np.dtype(expect).name if expect is not None else 'an integer column'}")


def _check_values(values, kinds):
    values, kinds = list(values), list(kinds)
    if len(values) != len(kinds):
        raise ValueError(f"{len(values)} value columns and {len(kinds)} kinds")
    if len(values) > MAX_VALUES:
        raise ValueError(f"{len(values)} value columns: one folding call takes at most {MAX_VALUES}")
    codes = []
    for k, (v, kind) in enumerate(zip(values, kinds)):
        if kind not in KINDS:
            raise ValueError(f"value column {k}: the fold kind {kind!r} is not one of {sorted(KINDS)}")
        _check_typed(v, f"value column {k}", "iu", None)   # a Float column: the reference's sequential sum rounds differently from a scan
        codes.append(KINDS[kind])
    return values, codes


def _flags(check):
    return K.MERGE_CHECK_SORTED if check else 0


def _handle(ctx, cols, c):
    """the handle of an argument column, uploaded to the keys' context (kept alive in cols)"""
    c = ctx.column(c)
    cols.append(c)
    return c._h


def _check_replacing(version, is_deleted, column=lambda c, what: c):
    """Replacing's version / is_deleted pair, None: absent.  column(argument, what) is the column an argument names: the argument itself
    for the rows form, the first block's column at that position for the Block form."""
    if version is not None:
        _check_typed(column(version, "the version"), "the version column", "iu", None)
    if is_deleted is not None:
        if version is None:
            raise ValueError("is_deleted without a version column is not implemented")
        _check_typed(column(is_deleted, "the is_deleted"), "the is_deleted column", "u", np.uint8)


def replacing_merge_rows(key_cols, description, run_offsets, version=None, is_deleted=None, cleanup: bool = False, check: bool = True) -> Column:
    """per group of equal keys the last row in merged order among those of the greatest version (without a version: the group's last
    row) -> the UInt64 Column of their concatenated row numbers.  is_deleted (UInt8, needs a version): with cleanup a group whose
    selected row is deleted emits nothing."""
    _check_replacing(version, is_deleted)
    ctx, cols, args = _prepare(key_cols, description, run_offsets)
    v = _handle(ctx, cols, version) if version is not None else None
    d = _handle(ctx, cols, is_deleted) if is_deleted is not None else None
    out = C.c_void_p()
    K.check(K.lib().chgpu_merge_replacing(ctx._live(), *args, _flags(check), v, d, 1 if cleanup else 0, C.byref(out)))
    return Column(ctx, out)


def _sign_merge_rows(entry, key_cols, description, run_offsets, sign, check, *more_outputs):
    """the two merges by an Int8 sign: the sign checked, the keys prepared, the sign uploaded beside them, `entry` called -> the rows"""
    _check_typed(sign, "the sign column", "i", np.int8)
    ctx, cols, args = _prepare(key_cols, description, run_offsets)
    s = _handle(ctx, cols, sign)
    out = C.c_void_p()
    K.check(getattr(K.lib(), entry)(ctx._live(), *args, _flags(check), s, C.byref(out), *more_outputs))
    return Column(ctx, out)


def collapsing_merge_rows(key_cols, description, run_offsets, sign, check: bool = True) -> Column:
    """CollapsingSortedAlgorithm: per group nothing, the first negative row, the last positive row, or both -> their row numbers"""
    return _sign_merge_rows("chgpu_merge_collapsing", key_cols, description, run_offsets, sign, check)


def versioned_collapsing_merge_rows(key_cols, description, run_offsets, sign, check: bool = True):
    """VersionedCollapsingAlgorithm: the version is the last key column, so a group is equal on the key and the version; within it a
    row cancels the nearest unmatched earlier row of the other sign and every unmatched row survives (|cp - cn| rows of the majority
    sign) -> (their row numbers, max_balance).  The queue is unbounded: the answer is the reference's whenever max_balance, the largest
    number of rows its queue would have held, is below the reference's max_rows_in_queue."""
    balance = C.c_uint64(0)
    rows = _sign_merge_rows("chgpu_merge_versioned_collapsing", key_cols, description, run_offsets, sign, check, C.byref(balance))
    return rows, int(balance.value)


def aggregating_merge_rows(key_cols, description, run_offsets, values, kinds, drop_zero: bool = False, check: bool = True):
    """values[i] folded by kinds[i] in ("sum", "min", "max") per group of equal keys
    -> (first_rows, last_rows, [result Column per value]); drop_zero: Summing's rule"""
    values, codes = _check_values(values, kinds)
    ctx, cols, args = _prepare(key_cols, description, run_offsets)
    n = len(values)
    handles = (C.c_void_p * max(n, 1))(*[_handle(ctx, cols, v) for v in values])
    first, last = C.c_void_p(), C.c_void_p()
    res = (C.c_void_p * max(n, 1))()
    K.check(K.lib().chgpu_merge_folding(ctx._live(), *args, _flags(check), handles, (C.c_int32 * max(n, 1))(*codes), n, 1 if drop_zero else 0, C.byref(first),
                                        C.byref(last), res))
    return Column(ctx, first), Column(ctx, last), [Column(ctx, C.c_void_p(res[k])) for k in range(n)]


def summing_merge_rows(key_cols, description, run_offsets, values, check: bool = True):
    """SummingSortedAlgorithm: every value column summed with wrap-around, groups whose sums are all 0 dropped"""
    values = list(values)
    return aggregating_merge_rows(key_cols, description, run_offsets, values, ["sum"] * len(values), drop_zero=True, check=check)


def _position(pos, width, what):
    if not isinstance(pos, (int, np.integer)) or not 0 <= pos < width:
        raise ValueError(f"{what} position {pos!r} is not one of the {width} columns")
    return int(pos)


def replacing_merge(blocks, description, version=None, is_deleted=None, cleanup: bool = False, check: bool = True):
    """ReplacingSortedTransform over sorted Blocks; version / is_deleted are column positions.  -> (columns, rows)"""
    glued, description, offsets, _ = _glue_blocks(
        blocks, description, lambda first, width, _: _check_replacing(version, is_deleted, lambda pos, what: first[_position(pos, width, what)]))
    rows = replacing_merge_rows(glued, description, offsets, None if version is None else glued[version], None if is_deleted is None else glued[is_deleted],
                                cleanup=cleanup, check=check)
    return [c.index(rows) for c in glued], rows


def _sign_merge(merge_rows, blocks, description, sign, check):
    """-> (the glued columns, what merge_rows answers for them with the Int8 sign column at position `sign`)"""
    glued, description, offsets, _ = _glue_blocks(
        blocks, description, lambda first, width, _: _check_typed(first[_position(sign, width, "the sign")], "the sign column", "i", np.int8))
    return glued, merge_rows(glued, description, offsets, glued[sign], check=check)


def collapsing_merge(blocks, description, sign, check: bool = True):
    """CollapsingSortedTransform over sorted Blocks; sign is the position of the Int8 sign column.  -> (columns, rows)"""
    glued, rows = _sign_merge(collapsing_merge_rows, blocks, description, sign, check)
    return [c.index(rows) for c in glued], rows


def versioned_collapsing_merge(blocks, description, sign, check: bool = True):
    """VersionedCollapsingTransform over sorted Blocks; the description ends with the version column, sign is the position of the Int8
    sign column.  -> (columns, rows, max_balance)"""
    glued, (rows, balance) = _sign_merge(versioned_collapsing_merge_rows, blocks, description, sign, check)
    return [c.index(rows) for c in glued], rows, balance


def _folding_merge(blocks, description, kinds_of, drop_zero, check):
    """kinds_of(first block, width, key positions) -> {position: "sum" | "min" | "max" | "any" | "anyLast"}; every other column is `any`"""
    def check_layout(first, width, description):
        kinds = kinds_of(first, width, {pos for pos, _, _ in description})
        folded = [p for p in sorted(kinds) if kinds[p] in KINDS]
        for p in folded:
            _check_typed(first[p], f"column {p}", "iu", None)
        if len(folded) > MAX_VALUES:
            raise ValueError(f"{len(folded)} folded columns: one folding call takes at most {MAX_VALUES}")
        return kinds, folded

    glued, description, offsets, (kinds, folded) = _glue_blocks(blocks, description, check_layout)
    first, last, results = aggregating_merge_rows(glued, description, offsets, [glued[p] for p in folded], [kinds[p] for p in folded], drop_zero=drop_zero,
                                                  check=check)
    out = []
    for p in range(len(glued)):
        if p in folded:
            out.append(results[folded.index(p)])
        else:
            out.append(glued[p].index(last if kinds.get(p) == "anyLast" else first))
    return out, first


def summing_merge(blocks, description, columns_to_sum=None, check: bool = True):
    """SummingSortedTransform over sorted Blocks: columns_to_sum (positions) summed, None: every integer column that is not a key; every
    other column is the group's first row's.  -> (columns, first_rows)"""
    def kinds_of(first, width, key_positions):
        positions = columns_to_sum
        if positions is None:
            positions = [p for p in range(width) if p not in key_positions and _dtype_of(first[p]).kind in "iu"]
        positions = [_position(p, width, "a summed column's") for p in positions]
        if any(p in key_positions for p in positions):
            raise ValueError("a key column cannot be summed")
        return {p: "sum" for p in positions}

    return _folding_merge(blocks, description, kinds_of, True, check)


def aggregating_merge(blocks, description, kinds, check: bool = True):
    """AggregatingSortedTransform over SimpleAggregateFunction columns: kinds = {position: "sum" | "min" | "max" | "any" | "anyLast"};
    keys and every column not named are `any`.  -> (columns, first_rows)"""
    def kinds_of(first, width, key_positions):
        checked = {_position(p, width, "a folded column's"): k for p, k in dict(kinds).items()}
        for p, k in checked.items():
            if k not in KINDS and k not in ("any", "anyLast"):
                raise ValueError(f"column {p}: {k!r} is not one of sum, min, max, any, anyLast")
            if p in key_positions:
                raise ValueError(f"column {p} is a key column: it cannot be folded")
        return checked

    return _folding_merge(blocks, description, kinds_of, False, check)
