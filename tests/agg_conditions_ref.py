"""The -If combinator and Nullable arguments of the GROUP BY aggregates restated in row order, plain numpy and Python: per group and
function, the rows in block order, filtered by the WHERE mask and then by the function's own condition, folded with the reference's
rule (AggregateFunctionIf::add, AggregateFunctionNullUnary::add, AggregateFunctionCountNotNullUnary::add over the nested function).

    mode None    every row that passes WHERE reaches the function
    mode "if"    ... whose condition byte is non-zero (any non-zero value).  No row reached it: count 0, sum 0 (Float: +0.0), avg NaN,
                 min / max / any / argMin / argMax the type's default
    mode "null"  ... whose null-map byte is zero.  The result is Nullable: (value, null flag); no row reached it: flag 1 and the type's
                 default as the nested value (avg: 0.0, not NaN).  count has no flag.

A group exists as soon as one of its rows passes WHERE, whatever the conditions say (the key is emplaced before any add).
Integer sums wrap modulo 2^64, Float sums are math.fsum of the rows as Float64 (the device's deterministic sums equal it whenever the
values fit its fixed-point window exactly, which the tests arrange), avg = Float64(sum) / count.  any takes the first row that reaches
it, argMin / argMax the first such row that holds the extremum.  min / max and the val of argMin / argMax are ordered by the device's
documented order key (tests/arg_min_max_ref.py): a total order, -0.0 below +0.0 for min / max.

This module is the reference of tests/test_gpu_agg_conditions.py; tests/test_agg_conditions_ref.py pins it on hand-written rows.
tests/golden holds no -If / Nullable rows: parity with the reference implementation rests on this restatement alone."""
import math

import numpy as np

import arg_min_max_ref as A

COUNT, SUM, AVG, MIN, MAX, ANY, ARG_MIN, ARG_MAX = range(8)
M64 = (1 << 64) - 1


def order_key(x):
    """min / max: the value mapped to an unsigned integer that sorts like it (no folding of the zero's sign)"""
    v = np.asarray(x)
    if v.dtype.kind == "f":
        bits = int(v.astype(np.float64).view(np.uint64))
        return (~bits & M64) if bits >> 63 else bits ^ (1 << 63)
    if v.dtype.kind == "i":
        return (int(v) + (1 << 63)) & M64
    return int(v)


def sum_dtype(dt):
    dt = np.dtype(dt)
    return np.dtype(np.float64) if dt.kind == "f" else np.dtype(np.int64) if dt.kind == "i" else np.dtype(np.uint64)


class FnState:
    """one function's state of one group"""
    __slots__ = ("kind", "n", "isum", "fvals", "best", "key", "arg")

    def __init__(self, kind):
        self.kind, self.n, self.isum, self.fvals, self.best, self.key, self.arg = kind, 0, 0, [], None, 0, A.State()

    def add(self, x, val_key=None):
        """x: the row's argument as a numpy scalar (count: None); val_key: argMin / argMax's order key of val"""
        k = self.kind
        if k in (SUM, AVG):
            if x.dtype.kind == "f":
                self.fvals.append(float(x))
            else:
                self.isum = (self.isum + int(x)) & M64
        elif k in (MIN, MAX):
            key = order_key(x)
            key = (~key & M64) if k == MIN else key
            if self.n == 0 or key > self.key:
                self.best, self.key = x, key
        elif k == ANY:
            if self.n == 0:
                self.best = x
        elif k in (ARG_MIN, ARG_MAX):
            self.arg.add(val_key, x)
        self.n += 1

    def merge(self, o):
        """the nested function's merge; the row counts add (the `seen` word, avg's denominator, count)"""
        k = self.kind
        if k in (SUM, AVG):
            self.isum = (self.isum + o.isum) & M64
            self.fvals += o.fvals
        elif k in (MIN, MAX):
            if o.n and (self.n == 0 or o.key > self.key):
                self.best, self.key = o.best, o.key
        elif k == ANY:
            if self.n == 0 and o.n:
                self.best = o.best
        elif k in (ARG_MIN, ARG_MAX):
            self.arg.merge(o.arg)
        self.n += o.n


class Ref:
    """aggs: [(kind, arg dtype | (arg dtype, val dtype) | None, mode)], as clickhouse_amd.Aggregator takes them"""

    def __init__(self, aggs):
        self.aggs = [(e[0], e[1], e[2] if len(e) > 2 else None) for e in aggs]
        self.groups = {}     # key -> [FnState]; insertion order = first appearance
        self.overflow = None  # the overflow row's [FnState], once a find-only block ran with one

    def _new(self):
        return [FnState(k) for k, _, _ in self.aggs]

    def add_block(self, keys, args, conds=None, where=None, row_begin=0, row_end=None, find_only=False, overflow_row=False):
        """keys None = without key (one group, key None, which always exists after the first block).  find_only: a no_more_keys block --
        rows of absent keys go to the overflow row (overflow_row) or are dropped."""
        cols = [tuple(np.asarray(x) for x in a) if isinstance(a, tuple) else (np.asarray(a) if a is not None else None) for a in args]
        conds = [None] * len(self.aggs) if conds is None else [np.asarray(c) if c is not None else None for c in conds]
        n = len(keys) if keys is not None else max(len(c[0] if isinstance(c, tuple) else c) for c in cols + conds if c is not None)
        row_end = n if row_end is None else row_end
        vkeys = [A.val_keys(c[1], k == ARG_MIN) if k in (ARG_MIN, ARG_MAX) else None for (k, _, _), c in zip(self.aggs, cols)]
        if keys is None:
            self.groups.setdefault(None, self._new())
        if overflow_row and self.overflow is None:
            self.overflow = self._new()
        kl = None if keys is None else [int(k) for k in np.asarray(keys)]
        for i in range(row_begin, row_end):
            if where is not None and not where[i]:
                continue
            key = None if kl is None else kl[i]
            st = self.groups.get(key)
            if st is None:
                if find_only:
                    st = self.overflow if overflow_row else None
                    if st is None:
                        continue
                else:
                    st = self.groups[key] = self._new()
            for j, (kind, _, mode) in enumerate(self.aggs):
                if mode == "if" and not conds[j][i]:
                    continue
                if mode == "null" and conds[j][i]:
                    continue
                c = cols[j]
                if kind == COUNT:
                    st[j].add(None)
                elif kind in (ARG_MIN, ARG_MAX):
                    st[j].add(c[0][i], vkeys[j][i])
                else:
                    st[j].add(c[i])

    def merge(self, other):
        """mergeDataImpl: every group of `other`, also one that no function has a row for"""
        for key, src in other.groups.items():
            dst = self.groups.setdefault(key, self._new())
            for d, s in zip(dst, src):
                d.merge(s)

    def result_dtype(self, j):
        kind, dt, _ = self.aggs[j]
        if kind == COUNT:
            return np.dtype(np.uint64)
        if kind == AVG:
            return np.dtype(np.float64)
        if kind == SUM:
            return sum_dtype(dt)
        return np.dtype(dt[0] if kind in (ARG_MIN, ARG_MAX) else dt)

    def value_of(self, j, st):
        """(nested value as a numpy scalar of the result type, null flag or None) of function j's state"""
        kind, dt, mode = self.aggs[j]
        rt = self.result_dtype(j)
        null = None if (mode != "null" or kind == COUNT) else int(st.n == 0)
        if kind == COUNT:
            return rt.type(st.n), null
        if kind in (SUM, AVG):
            if np.dtype(dt).kind == "f":
                s = math.fsum(st.fvals)
            else:
                s = st.isum - (1 << 64) if (np.dtype(dt).kind == "i" and st.isum >> 63) else st.isum
            if kind == SUM:
                return (rt.type(s) if rt.kind == "f" else np.array(s & M64, dtype=np.uint64).astype(rt)[()]), null
            if st.n == 0:
                return np.float64(0.0 if mode == "null" else np.nan), null
            return np.float64(float(s) / st.n), null
        if kind in (ARG_MIN, ARG_MAX):
            return (rt.type(st.arg.arg) if st.arg.has else rt.type(0)), null
        return (rt.type(st.best) if st.n else rt.type(0)), null

    def columns(self, key_order):
        """for the groups in `key_order`: ([value ndarray per function], [null-map ndarray or None per function])"""
        vals, nulls = [], []
        for j in range(len(self.aggs)):
            got = [self.value_of(j, self.groups[None if k is None else int(k)][j]) for k in key_order]
            vals.append(np.array([v for v, _ in got], dtype=self.result_dtype(j)))
            nulls.append(None if (not got or got[0][1] is None) else np.array([f for _, f in got], dtype=np.uint8))
        if not len(key_order):
            nulls = [None if (m != "null" or k == COUNT) else np.zeros(0, dtype=np.uint8) for k, _, m in self.aggs]
        return vals, nulls

    def overflow_columns(self):
        vals, nulls = [], []
        for j in range(len(self.aggs)):
            v, f = self.value_of(j, self.overflow[j])
            vals.append(np.array([v], dtype=self.result_dtype(j)))
            nulls.append(None if f is None else np.array([f], dtype=np.uint8))
        return vals, nulls


def additive_reference(keys, args, conds, aggs, where=None):
    """One block of count / sum / avg over INTEGER arguments, vectorised (the large shapes): (group keys ascending, [value ndarray per
    function], [null-map or None]).  The same rule as Ref: every key that passes WHERE is a group."""
    keys = np.asarray(keys)
    live = np.ones(len(keys), dtype=bool) if where is None else np.asarray(where) != 0
    gk, inv = np.unique(keys[live], return_inverse=True)
    vals, nulls = [], []
    for (kind, dt, *m), a, c in zip(aggs, args, conds):
        mode = m[0] if m else None
        reach = np.ones(len(keys), dtype=bool) if mode is None else (np.asarray(c) != 0) if mode == "if" else (np.asarray(c) == 0)
        reach = reach[live]
        cnt = np.bincount(inv[reach], minlength=len(gk)).astype(np.uint64)
        null = None if (mode != "null" or kind == COUNT) else (cnt == 0).astype(np.uint8)
        if kind == COUNT:
            vals.append(cnt), nulls.append(null)
            continue
        assert kind in (SUM, AVG) and np.dtype(dt).kind in "iu"
        s = np.zeros(len(gk), dtype=np.uint64)
        x = np.asarray(a)[live][reach]
        np.add.at(s, inv[reach], x.astype(np.int64).view(np.uint64) if x.dtype.kind == "i" else x.astype(np.uint64))  # wraps modulo 2^64
        s = s.view(np.int64) if np.dtype(dt).kind == "i" else s
        if kind == SUM:
            vals.append(s.copy())
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                q = s.astype(np.float64) / cnt.astype(np.float64)
            if mode == "null":
                q[cnt == 0] = 0.0
            vals.append(q)
        nulls.append(null)
    return gk, vals, nulls
