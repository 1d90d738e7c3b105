"""The merge of sorted runs over the C ABI: MergingSortedTransform (MergingSortedAlgorithm over SortCursor,
src/Processors/Merges/Algorithms/MergingSortedAlgorithm.cpp) and MergeSortingTransform (src/Processors/Transforms/MergeSortingTransform.cpp)
without the spill, and isAlreadySorted (src/Interpreters/sortBlock.cpp).  The key columns are the runs glued end to end; the answer is the
permutation sort_block gives for the concatenation under the same description -- by merging, not by sorting again.  Numeric keys only: a
ColumnString as a key or as a carried column raises TypeError before the library is touched."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from .columns import TAG_OF, Column, Context, concat, sort_block
from .lowcardinality import ColumnLowCardinality, ColumnString

TILE = 2048      # T: outputs of one merge tile (MRG_TILE of csrc/merge_host.h)
MAX_KEYS = 8
MAX_ROWS = 2**32 - 1


def _check_column(c, what):
    if isinstance(c, (ColumnString, ColumnLowCardinality)):
        raise TypeError(f"{what} is a {type(c).__name__}: the merge of sorted runs takes numeric columns only")
    if isinstance(c, Column):
        return
    try:
        TAG_OF[np.asarray(c).dtype]
    except (KeyError, TypeError):
        raise TypeError(f"{what} dtype {getattr(c, 'dtype', type(c))!r} is not one of the column types") from None


def _check_description(description, n_columns):
    """[(position, descending, nan_direction_hint), ...] as sort_block takes it -> the same as a list of int triples"""
    description = [tuple(d) for d in description]
    if not 1 <= len(description) <= MAX_KEYS:
        raise ValueError(f"a sort description has 1 to {MAX_KEYS} columns, not {len(description)}")
    out = []
    for d in description:
        if len(d) != 3:
            raise ValueError(f"a sort description entry is (position, descending, nan_direction_hint), not {d!r}")
        pos, desc, hint = d
        if not isinstance(pos, (int, np.integer)) or not 0 <= pos < n_columns:
            raise ValueError(f"sort description position {pos!r} is not one of the {n_columns} columns")
        if hint not in (1, -1):
            raise ValueError(f"nan_direction_hint {hint!r} is neither 1 nor -1")
        out.append((int(pos), 1 if desc else 0, int(hint)))
    return out


def _check_offsets(run_offsets, rows):
    offs = [int(x) for x in run_offsets]
    if not offs or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError("run offsets are cumulative: they start at 0 and never decrease")
    if offs[-1] != rows:
        raise ValueError(f"the run offsets end at {offs[-1]}, the key columns have {rows} rows")
    if rows > MAX_ROWS:
        raise ValueError(f"{rows} rows: a merge takes at most {MAX_ROWS}")
    return offs


def _prepare(key_cols, description, run_offsets):
    key_cols = list(key_cols)
    for k, c in enumerate(key_cols):
        _check_column(c, f"key column {k}")
    description = _check_description(description, len(key_cols))
    rows = len(key_cols[description[0][0]])
    if any(len(key_cols[pos]) != rows for pos, _, _ in description):
        raise ValueError("key columns of different lengths")
    offs = _check_offsets([0, rows] if run_offsets is None else run_offsets, rows)
    ctx = next((c.ctx for c in key_cols if isinstance(c, Column)), None) or Context(0)
    cols = [ctx.column(key_cols[pos]) for pos, _, _ in description]
    n = len(cols)
    args = ((C.c_void_p * n)(*[c._h for c in cols]), (C.c_int32 * n)(*[d for _, d, _ in description]), (C.c_int32 * n)(*[h for _, _, h in description]), n,
            (C.c_uint64 * len(offs))(*offs), len(offs) - 1)
    return ctx, cols, args


def is_sorted(key_cols, description, run_offsets=None):
    """None when every run is sorted under the description, else the lowest concatenated row number that orders strictly before its
    predecessor inside one run.  description positions index key_cols; run_offsets None: one run."""
    ctx, cols, args = _prepare(key_cols, description, run_offsets)
    row = C.c_uint64(0)
    K.check(K.lib().chgpu_is_sorted(ctx._live(), *args, C.byref(row)))
    return None if row.value == 2**64 - 1 else int(row.value)


def merge_sorted_permutation(key_cols, description, run_offsets, limit: int = 0, check: bool = True) -> Column:
    """the stable merge of the runs as a UInt64 permutation Column of concatenated row numbers (the first `limit` entries when given).
    check: an unsorted run raises ChgpuError(ERR_BAD_ARGUMENTS); without it the order is then unspecified."""
    if limit < 0:
        raise ValueError(f"limit {limit!r} must not be negative")
    ctx, cols, args = _prepare(key_cols, description, run_offsets)
    out = C.c_void_p()
    K.check(K.lib().chgpu_merge_sorted_permutation(ctx._live(), *args, int(limit), K.MERGE_CHECK_SORTED if check else 0, C.byref(out)))
    return Column(ctx, out)


def _check_blocks(blocks):
    blocks = [list(b) for b in blocks]
    if not blocks:
        raise ValueError("no blocks to merge")
    width = len(blocks[0])
    for b, block in enumerate(blocks):
        if len(block) != width:
            raise ValueError(f"block {b} has {len(block)} columns, block 0 has {width}")
        for k, c in enumerate(block):
            _check_column(c, f"column {k} of block {b}")
        if any(len(c) != len(block[0]) for c in block):
            raise ValueError(f"block {b} has columns of different lengths")
    return blocks, width


def _glue_blocks(blocks, description, check_layout=None):
    """Sorted Blocks (each a list of Columns / arrays) as what the *_rows functions take: the blocks and the description are checked,
    then check_layout(first block, width, description) raises for what its caller asks of the layout -- all of that before the
    library is touched -- and the blocks are uploaded to one context and concatenated column by column.
    -> (glued columns, description, run offsets, what check_layout returned)"""
    blocks, width = _check_blocks(blocks)
    description = _check_description(description, width)
    layout = check_layout(blocks[0], width, description) if check_layout is not None else None
    ctx = next((c.ctx for block in blocks for c in block if isinstance(c, Column)), None) or Context(0)
    blocks = [[ctx.column(c) for c in block] for block in blocks]
    offsets = [0]
    for block in blocks:
        offsets.append(offsets[-1] + (len(block[0]) if block else 0))
    return [concat([block[k] for block in blocks]) for k in range(width)], description, offsets, layout


def merge_sorted_blocks(blocks, description, limit: int = 0, check: bool = True):
    """MergingSortedTransform over sorted Blocks (each a list of Columns / arrays): concatenates every column, merges by the description
    (that of sort_block) and indexes every column.  -> (columns, perm)"""
    glued, description, offsets, _ = _glue_blocks(blocks, description)
    perm = merge_sorted_permutation(glued, description, offsets, limit=limit, check=check)
    return [c.index(perm) for c in glued], perm


class MergeSorting:
    """MergeSortingTransform without the spill: add_block sorts a block as it arrives (cut to the limit) and keeps it, finish merges
    the sorted blocks."""

    def __init__(self, description, limit: int = 0, ctx: Context | None = None):
        self.description = [tuple(d) for d in description]
        if limit < 0:
            raise ValueError(f"limit {limit!r} must not be negative")
        self.limit = int(limit)
        self.ctx = ctx
        self.blocks = []

    def add_block(self, columns):
        columns = list(columns)
        for k, c in enumerate(columns):
            _check_column(c, f"column {k}")
        _check_description(self.description, len(columns))
        if self.ctx is None:
            self.ctx = next((c.ctx for c in columns if isinstance(c, Column)), None) or Context(0)
        columns = [self.ctx.column(c) for c in columns]
        if len(columns[0]) == 0:
            return
        sorted_columns, _ = sort_block(columns, self.description, self.limit)
        self.blocks.append(sorted_columns)

    def finish(self):
        """-> the merged columns (the first `limit` rows when given); None when no row was added"""
        if not self.blocks:
            return None
        # the blocks were sorted here: nothing to check
        columns, _ = merge_sorted_blocks(self.blocks, self.description, limit=self.limit, check=False)
        self.blocks = []
        return columns
