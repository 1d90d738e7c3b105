"""Aggregator mirror (src/Interpreters/Aggregator.h:179-265) over the C ABI: one instance == one
AggregatedDataVariants living in HBM.  execute_on_block / merge / convert_to_block follow executeOnBlock /
mergeDataImpl / convertToBlockImplFinal."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from .columns import NP_OF, TAG_OF, Column, Context, sum_result_dtype


_OVERFLOW_MODES = {"throw": K.OVERFLOW_THROW, "break": K.OVERFLOW_BREAK, "any": K.OVERFLOW_ANY}
_TWO_ARGS = (K.AGG_ARG_MIN, K.AGG_ARG_MAX)   # argMin(arg, val) / argMax(arg, val): two argument slots of the C ABI, arg then val
# the third element of an `aggs` entry: "if" = the -If combinator, "null" = a Nullable(T) argument (chgpu_agg_set_conditions)
_COND_MODES = {None: K.AGG_COND_NONE, "if": K.AGG_COND_IF, "null": K.AGG_COND_NULL}


class Aggregator:
    def __init__(self, key_dtype, aggs, two_level_threshold: int = 100000, size_hint: int = 0, ctx: Context | None = None,
                 max_rows_to_group_by: int = 0, group_by_overflow_mode: str = "throw", overflow_row: bool = False):
        """aggs: list of (kind, arg_dtype or None); argMin / argMax: (kind, (arg_dtype, val_dtype)), and the matching entry of
        execute_on_block's args is (arg_array, val_array).  An entry may carry a third element, "if" or "null": the function then
        takes one UInt8 column of execute_on_block's conds, a condition ("if": rows whose byte is non-zero reach it) or a null map
        ("null": rows whose byte is zero reach it, the result is Nullable).  key_dtype None = without_key.  two_level_threshold is accepted for
        interface parity (Aggregator::Params) — the device table is single-level.  max_rows_to_group_by (0 = no limit),
        group_by_overflow_mode ("throw" / "break" / "any") and overflow_row are the settings of the same names."""
        mode = _OVERFLOW_MODES.get(group_by_overflow_mode)
        if mode is None:
            raise ValueError(f"group_by_overflow_mode must be one of {sorted(_OVERFLOW_MODES)}, not {group_by_overflow_mode!r}")
        self.ctx = ctx if ctx is not None else Context(0)
        self.key_tag = -1 if key_dtype is None else TAG_OF[np.dtype(key_dtype)]
        for e in aggs:
            if len(e) > 2 and e[2] not in _COND_MODES:
                raise ValueError(f"the condition of an aggregate is 'if' or 'null', not {e[2]!r}")
        self.cond_modes = [_COND_MODES[e[2] if len(e) > 2 else None] for e in aggs]
        self.conditioned = any(self.cond_modes)
        aggs = [(e[0], e[1]) for e in aggs]
        # (kind, tag of the result's argument); val_tags[j]: the second argument's tag of a two-argument function, else None
        self.aggs = [(k, (TAG_OF[np.dtype(d[0] if k in _TWO_ARGS else d)] if d is not None else K.U64)) for k, d in aggs]
        self.val_tags = [TAG_OF[np.dtype(d[1])] if k in _TWO_ARGS else None for k, d in aggs]
        slots = [t for (_, t), v in zip(self.aggs, self.val_tags) for t in ((t,) if v is None else (t, v))]
        kinds = (C.c_int * max(1, len(self.aggs)))(*[k for k, _ in self.aggs])
        types = (C.c_int * max(1, len(slots)))(*slots)
        h = C.c_void_p()
        K.check(K.lib().chgpu_agg_create(self.ctx._h, self.key_tag, len(self.aggs), kinds, types, size_hint, C.byref(h)))
        self._h = h
        self.limited = bool(max_rows_to_group_by) or bool(overflow_row)
        self.no_more_keys = False   # AggregatingTransform's, one per stream: this instance is one stream's variants
        if self.limited:
            K.check(K.lib().chgpu_agg_set_limits(self._h, int(max_rows_to_group_by), mode, int(bool(overflow_row))))
        if self.conditioned:
            K.check(K.lib().chgpu_agg_set_conditions(self._h, (C.c_int * len(self.cond_modes))(*self.cond_modes)))

    def close(self):
        if getattr(self, "_h", None):
            K.lib().chgpu_agg_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def execute_on_block(self, keys, args, row_begin: int = 0, row_end: int | None = None, filter=None, conds=None):
        """Aggregator::executeOnBlock(columns, row_begin, row_end, result, key_columns, aggregate_columns, ...).
        filter: a UInt8 WHERE mask over the same rows (a FilterTransform fused in front of the aggregation).
        conds: one UInt8 array / Column or None per aggregate, the condition or null map of the "if" / "null" entries."""
        kcol = self.ctx.column(keys) if keys is not None else None
        # one column per argument slot: a two-argument function's (arg, val) pair takes two
        flat = [x for (k, _), a in zip(self.aggs, args) for x in (a if k in _TWO_ARGS else (a,))]
        acols = [self.ctx.column(a) if a is not None else None for a in flat]
        fcol = self.ctx.column(filter) if filter is not None else None
        n = kcol.size() if kcol is not None else (fcol.size() if fcol is not None else next(a.size() for a in acols if a is not None))
        row_end = n if row_end is None else row_end
        ptrs = (C.c_void_p * max(1, len(acols)))(*[(a._h if a is not None else None) for a in acols])
        if self.conditioned or conds is not None:
            ccols = [self.ctx.column(c) if c is not None else None for c in (conds if conds is not None else [None] * len(self.aggs))]
            if len(ccols) != len(self.aggs):
                raise ValueError(f"conds has {len(ccols)} entries for {len(self.aggs)} aggregates")
            cptrs = (C.c_void_p * max(1, len(ccols)))(*[(c._h if c is not None else None) for c in ccols])
            nmk, keep = C.c_int(int(self.no_more_keys)), C.c_int(1)
            K.check(K.lib().chgpu_agg_execute_on_block_conditional(
                self._h, kcol._h if kcol is not None else None, ptrs, cptrs, row_begin, row_end, fcol._h if fcol is not None else None,
                C.byref(nmk) if self.limited else None, C.byref(keep) if self.limited else None))
            self.no_more_keys = bool(nmk.value)
            return bool(keep.value)
        if self.limited:
            # -> False on group_by_overflow_mode BREAK ("stop reading"); ANY sets self.no_more_keys; THROW raises ERR_TOO_MANY_ROWS
            nmk, keep = C.c_int(int(self.no_more_keys)), C.c_int(1)
            K.check(K.lib().chgpu_agg_execute_on_block(self._h, kcol._h if kcol is not None else None, ptrs, row_begin, row_end,
                                                       fcol._h if fcol is not None else None, C.byref(nmk), C.byref(keep)))
            self.no_more_keys = bool(nmk.value)
            return bool(keep.value)
        if fcol is None:
            K.check(K.lib().chgpu_agg_add_block(self._h, kcol._h if kcol is not None else None, ptrs, row_begin, row_end))
        else:
            K.check(K.lib().chgpu_agg_add_block_filtered(self._h, kcol._h if kcol is not None else None, ptrs, row_begin, row_end, fcol._h))
        return True

    def merge(self, other: "Aggregator", no_more_keys: bool = False) -> bool:
        """mergeDataImpl; under limits one step of mergeSingleLevelDataImpl (merge_limited): False = BREAK, stop merging keyed data.
        no_more_keys belongs to one sequence of merges (it is local to mergeSingleLevelDataImpl): pass False for its first step and,
        for each next one, the self.merge_no_more_keys the previous step left."""
        if not self.limited:
            K.check(K.lib().chgpu_agg_merge(self._h, other._h))
            return True
        nmk, keep = C.c_int(int(bool(no_more_keys))), C.c_int(1)
        K.check(K.lib().chgpu_agg_merge_limited(self._h, other._h, C.byref(nmk), C.byref(keep)))
        self.merge_no_more_keys = bool(nmk.value)
        return bool(keep.value)

    def merge_states(self, keys: Column | None, state_cols, rows: int, is_overflows: bool = False) -> bool:
        """mergeOnBlock; is_overflows: the one-row block of an overflow row.  -> False on BREAK."""
        ptrs = (C.c_void_p * max(1, len(state_cols)))(*[c._h for c in state_cols])
        if not self.limited and not is_overflows:
            K.check(K.lib().chgpu_agg_merge_states(self._h, keys._h if keys is not None else None, ptrs, rows))
            return True
        nmk, keep = C.c_int(int(self.no_more_keys)), C.c_int(1)
        K.check(K.lib().chgpu_agg_merge_states_limited(self._h, keys._h if keys is not None else None, ptrs, rows, int(bool(is_overflows)),
                                                       C.byref(nmk), C.byref(keep)))
        self.no_more_keys = bool(nmk.value)
        return bool(keep.value)

    def overflow_row(self, final: bool = True, null_maps: bool = False):
        """the overflow row: [one-row result Columns] (final) or [state word Columns]; None when there is none.
        null_maps (final only): -> ([result Columns], [one-row uint8 ndarray or None per aggregate]), the flags of the "null" entries
        read from the row's state words (no row reached the function <=> its seen word / denominator / claim is 0)."""
        n = len(self.aggs) if final else self.n_words
        res = (C.c_void_p * max(1, n))()
        has = C.c_int(0)
        K.check(K.lib().chgpu_agg_overflow_row(self._h, int(bool(final)), res, C.byref(has)))
        if not has.value:
            return None
        cols = [Column(self.ctx, C.c_void_p(res[k])) for k in range(n)]
        if not (final and null_maps):
            return cols
        words = Column.numpy_many(self.overflow_row(final=False))
        return cols, [np.array([words[w].view(np.uint64)[0] == 0], dtype=np.uint8) if w is not None else None for w in self._reached_words()]

    def _reached_words(self):
        """per aggregate: the state word that is 0 when no row reached a "null" function (None: not Nullable)"""
        out, w = [], 0
        for (k, _), m, nw in zip(self.aggs, self.cond_modes, self._words_per_agg()):
            out.append(None if m != K.AGG_COND_NULL or k == K.AGG_COUNT else w if k == K.AGG_ANY else w + 1)
            w += nw
        return out

    def convert_to_blocks(self, final: bool = True, null_maps: bool = False):
        """Aggregator::convertToBlocks: [merging.AggregatedBlock], the overflow row first (is_overflows, default key) when there is one.
        null_maps (final only): -> ([blocks], [per block: [uint8 ndarray or None per aggregate]])."""
        from .merging import AggregatedBlock
        out, maps = [], []
        ovf = self.overflow_row(final, null_maps=final and null_maps)
        if ovf is not None:
            if final and null_maps:
                ovf, m = ovf
                maps.append(m)
            kd = NP_OF[self.key_tag] if self.key_tag >= 0 else None
            out.append(AggregatedBlock(-1, True, (np.zeros(1, dtype=kd) if kd is not None else None), Column.numpy_many(ovf), 1))
        if final:
            got = self.convert_to_block(null_maps=null_maps)
            keys, res = got[:2]
            maps.append(got[2] if null_maps else None)
            out.append(AggregatedBlock(-1, False, keys, res, len(res[0]) if res else (len(keys) if keys is not None else 0)))
        else:
            kc, words, n = self.export_state_columns()
            out.append(AggregatedBlock(-1, False, kc.numpy() if kc is not None else None, Column.numpy_many(words) if words else [], n))
        return (out, maps) if (final and null_maps) else out

    def __len__(self):
        n = C.c_uint64(0)
        K.check(K.lib().chgpu_agg_size(self._h, C.byref(n)))
        return int(n.value)

    @property
    def n_words(self):
        return sum(self._words_per_agg())

    def _words_per_agg(self):
        # (min / max: one order-key word; any: claim + value; argMin / argMax: val word + has + arg bits; a conditioned min / max and a
        # "null" sum: one more, the number of rows that reached the function)
        return [(3 if k in _TWO_ARGS else 2 if k in (K.AGG_AVG, K.AGG_ANY) else 1)
                + int(m != K.AGG_COND_NONE and (k in (K.AGG_MIN, K.AGG_MAX) or (k == K.AGG_SUM and m == K.AGG_COND_NULL)))
                for (k, _), m in zip(self.aggs, getattr(self, "cond_modes", None) or [K.AGG_COND_NONE] * len(self.aggs))]

    def result_dtypes(self):
        out = []
        for kind, t in self.aggs:
            out.append(np.uint64 if kind == K.AGG_COUNT else np.float64 if kind == K.AGG_AVG else NP_OF[t] if kind in (K.AGG_MIN, K.AGG_MAX, K.AGG_ANY) + _TWO_ARGS else sum_result_dtype(t))
        return out

    def finalize_columns(self, null_maps: bool = False):
        """-> (keys Column or None, [result Columns]) resident in HBM; null_maps: a third element, [UInt8 Column or None per aggregate]
        (the null map of every "null" entry but count)."""
        kh = C.c_void_p()
        res = (C.c_void_p * max(1, len(self.aggs)))()
        n = C.c_uint64(0)
        if not null_maps:
            K.check(K.lib().chgpu_agg_finalize(self._h, C.byref(kh), res, C.byref(n)))
        else:
            maps = (C.c_void_p * max(1, len(self.aggs)))()
            K.check(K.lib().chgpu_agg_finalize_nullable(self._h, C.byref(kh), res, maps, C.byref(n)))
        keys = Column(self.ctx, kh) if kh.value else None
        cols = [Column(self.ctx, C.c_void_p(res[j])) for j in range(len(self.aggs))]
        if not null_maps:
            return keys, cols
        return keys, cols, [Column(self.ctx, C.c_void_p(maps[j])) if maps[j] else None for j in range(len(self.aggs))]

    def export_state_columns(self):
        kh = C.c_void_p()
        nw = self.n_words
        res = (C.c_void_p * max(1, nw))()
        n = C.c_uint64(0)
        K.check(K.lib().chgpu_agg_export_states(self._h, C.byref(kh), res, C.byref(n)))
        keys = Column(self.ctx, kh) if kh.value else None
        return keys, [Column(self.ctx, C.c_void_p(res[w])) for w in range(nw)], int(n.value)

    def export_state_columns_two_level(self):
        """the partial states ordered by two-level bucket number -> (keys, [state Columns], groups, bucket_counts[256])"""
        kh = C.c_void_p()
        nw = self.n_words
        res = (C.c_void_p * max(1, nw))()
        n = C.c_uint64(0)
        counts = (C.c_uint64 * 256)()
        K.check(K.lib().chgpu_agg_export_states_two_level(self._h, C.byref(kh), res, C.byref(n), counts))
        return Column(self.ctx, kh), [Column(self.ctx, C.c_void_p(res[w])) for w in range(nw)], int(n.value), [int(x) for x in counts]

    def convert_to_block(self, null_maps: bool = False):
        """Aggregator::convertToBlocks(final=true) downloaded: (keys ndarray or None, [result ndarrays]); null_maps: a third element,
        [uint8 ndarray or None per aggregate]."""
        if null_maps:
            keys, res, maps = self.finalize_columns(null_maps=True)
        else:
            (keys, res), maps = self.finalize_columns(), []
        live = [m for m in maps if m is not None]
        got = Column.numpy_many(([keys] if keys is not None else []) + res + live)   # one wait for the whole result Block
        k0 = 1 if keys is not None else 0
        out = (got[0] if keys is not None else None), got[k0:k0 + len(res)]
        if not null_maps:
            return out
        it = iter(got[k0 + len(res):])
        return out + ([next(it) if m is not None else None for m in maps],)


def serialize_states(ctx: Context, kind: int, word0: Column, word1: Column | None = None):
    """the ColumnAggregateFunction wire bytes of one aggregate function's states (IAggregateFunction::serialize per row: sum = 8 bytes,
    count = VarUInt, avg = 8 bytes + VarUInt) -> (bytes Column, row offsets Column[rows + 1])"""
    bh, oh = C.c_void_p(), C.c_void_p()
    K.check(K.lib().chgpu_agg_serialize_states(ctx._live(), kind, word0._h, word1._h if word1 is not None else None, C.byref(bh), C.byref(oh)))
    return Column(ctx, bh), Column(ctx, oh)


def deserialize_states(ctx: Context, kind: int, data: Column, stream_rows, stream_byte_begin=None):
    """the inverse, for mergeOnBlock: `stream_rows[s]` states from byte `stream_byte_begin[s]` of every stream -> (word0, word1 or None)"""
    n = len(stream_rows)
    rows = (C.c_uint64 * n)(*[int(r) for r in stream_rows])
    begin = (C.c_uint64 * n)(*[int(b) for b in stream_byte_begin]) if stream_byte_begin is not None else None
    h0, h1 = C.c_void_p(), C.c_void_p()
    K.check(K.lib().chgpu_agg_deserialize_states(ctx._live(), kind, data._h, n, begin, rows, C.byref(h0), C.byref(h1) if kind == K.AGG_AVG else None))
    return Column(ctx, h0), (Column(ctx, h1) if kind == K.AGG_AVG else None)


class NullableKeyAggregator:
    """GROUP BY a Nullable(T) key: AggregationDataWithNullKey (src/Interpreters/AggregatedData.h:71-95) keeps the NULL group's state
    out of the hash table (has_null_key_data / null_key_data), and the key extraction sends rows whose null-map byte is set there
    (ColumnsHashingImpl.h:196-240) whatever their nested value is.  Here: the hash table aggregates the rows whose null-map byte is 0
    (the WHERE-fused form of add_block, mask = NOT null), an aggregation without key takes the rows whose byte is set."""

    def __init__(self, key_dtype, aggs, ctx: Context | None = None, size_hint: int = 0):
        self.ctx = ctx if ctx is not None else Context(0)
        self.keyed = Aggregator(key_dtype, aggs, size_hint=size_hint, ctx=self.ctx)
        self.null_group = Aggregator(None, aggs, ctx=self.ctx)
        self.has_null_key_data = False
        from .expression import ActionsDAG
        d = ActionsDAG()
        d.add_function("not", d.add_input(0, np.uint8))
        self._not = d.compile()

    def execute_on_block(self, keys, null_map, args, conds=None):
        """keys: the nested column of the ColumnNullable, null_map: its UInt8 null map (ColumnNullable.h); conds: as Aggregator's"""
        from .columns import count_bytes_in_filter
        k = self.ctx.column(keys)
        nm = self.ctx.column(null_map)
        # (an argMin / argMax entry is an (arg, val) pair: both are uploaded once and shared by the two aggregations)
        acols = [tuple(self.ctx.column(x) for x in a) if isinstance(a, tuple) else self.ctx.column(a) if a is not None else None for a in args]
        not_null = self._not.execute(self.ctx, [nm], [1])[0]
        ccols = [self.ctx.column(c) if c is not None else None for c in conds] if conds is not None else None
        self.keyed.execute_on_block(k, acols, filter=not_null, conds=ccols)
        if count_bytes_in_filter(nm):
            self.has_null_key_data = True
            self.null_group.execute_on_block(None, acols, filter=nm, conds=ccols)

    def __len__(self):
        return len(self.keyed) + (1 if self.has_null_key_data else 0)

    def convert_to_block(self, null_maps: bool = False):
        """-> (keys ndarray, key null map ndarray[uint8], [result ndarrays]); the NULL group, when present, is the last row (the
        reference appends it the same way: insertDefault into the key column + 1 in the null map).  null_maps: a fourth element, the
        null map (or None) of every aggregate's result"""
        keys, res, *maps = self.keyed.convert_to_block(null_maps=null_maps)
        nulls = np.zeros(keys.shape[0], dtype=np.uint8)
        if self.has_null_key_data:
            _, nres, *nmaps = self.null_group.convert_to_block(null_maps=null_maps)
            keys = np.concatenate([keys, np.zeros(1, dtype=keys.dtype)])
            nulls = np.concatenate([nulls, np.ones(1, dtype=np.uint8)])
            res = [np.concatenate([r, n.astype(r.dtype)]) for r, n in zip(res, nres)]
            if null_maps:
                maps = [[np.concatenate([m, n]) if m is not None else None for m, n in zip(maps[0], nmaps[0])]]
        return (keys, nulls, res, maps[0]) if null_maps else (keys, nulls, res)


def group_by_min_max(ctx: Context, keys: Column, values: Column):
    """SELECT key, min(value), max(value) GROUP BY key ORDER BY key: min / max states in the hash aggregator (CHGPU_AGG_MIN / _MAX, round 3 --
    rounds 1-2 took a detour over two stable sorts), the groups then ordered by key.
    -> (keys Column, min Column, max Column), one row per group, ascending by key."""
    from .columns import sort_permutation
    if keys.size() == 0:
        return ctx.alloc(keys.dtype, 0), ctx.alloc(values.dtype, 0), ctx.alloc(values.dtype, 0)
    agg = Aggregator(keys.dtype, [(K.AGG_MIN, values.dtype), (K.AGG_MAX, values.dtype)], ctx=ctx)
    agg.execute_on_block(keys, [values, values])
    gk, (mn, mx) = agg.finalize_columns()
    perm = sort_permutation(gk)
    return gk.index(perm), mn.index(perm), mx.index(perm)
