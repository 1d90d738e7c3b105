"""Every instantiation of the fused filter / mask / sum kernels against the CPU oracle, at row counts taken from the kernels' geometry.

What runs on the device is picked at run time from the column type, the pointers' alignment, whether predicate and value are one
column, whether a mask came along and the comparison.  This module walks that whole matrix:

* k_filter_sum<T, VEC, SAME, HAS_COND, Pred> behind chgpu_filter_sum / _async / chgpu_sum_add_many / _conditional: ten types x
  {16-byte vectors, VEC = 1} x {TruePred with / without mask; IntRangePred or the six F64Pred<op>, one or two columns};
* k_cmp_mask<T, VEC, Pred> behind chgpu_cmp_const (and behind chgpu_filter_sum when predicate and value differ in type);
* k_expr_filter_sum<T>, all sixteen k_expr_filter_sum_narrow<WMASK> and k_expr_filter_sum_mixed behind chgpu_expr_filter_sum;
* the generated k_run behind chgpu_expr_filter_sum_node (ExpressionActions.filter_sum).

The reference is always the CPU oracle (cmp_const -> count_bytes_in_filter / sum_add_many_conditional, expr_filter_sum_pipeline) and,
where the case is small, Python integers or math.fsum as a second witness (tests/streaming_cases.py; checked without a device by
tests/test_streaming_cases.py).  Integer sums are compared bit for bit with the oracle's dtype.  Float columns are integer-valued
with |x| <= 2^20 and at most 2^25 rows, so every partial sum is exact in Float64 in any order and the device must match the oracle
bit for bit as well; the rounding path and the IEEE specials have their own tests.

That is everything instantiated: launch_filter_sum_t states which k_filter_sum combinations the C ABI can reach (a mask only ever
comes with TruePred over one column), and a chgpu_expr_filter_sum call whose columns are all UInt8 takes k_expr_filter_sum_narrow<0>.
A view that is not 16-byte aligned is refused by chgpu_expr_filter_sum, so the hand-fused kernels have no VEC = 1 form.

Row counts depend on the device's CU count, so they are looped over inside the tests; every assertion message carries the type,
the layout, the operator and the row count.
"""
import math

import numpy as np
import pytest

import streaming_cases as SC

pytestmark = pytest.mark.gpu

EQ, NE, LT, GT, LE, GE = range(6)
ALL_OPS = (EQ, NE, LT, GT, LE, GE)
I64, U32, U64, F64, U8, I32 = 0, 1, 2, 3, 4, 5


class Env:
    """the device context, the oracle and the columns of the matrix, each generated and uploaded once"""

    def __init__(self, ch, O):
        import torch
        self.ch, self.O = ch, O
        self.ctx = ch.Context(0)
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self._cols, self._masks, self._x, self._m = {}, {}, {}, None

    # -- filter / sum columns: pred (b) and val (a) per type, edge rows planted for every geometry of that type
    def pair(self, dtype):
        key = SC.name(dtype)
        if key not in self._cols:
            n = SC.max_rows(self.cus, dtype)
            geos = [SC.filter_sum_geometry(dtype, s, al, self.cus) for s in (True, False) for al in (True, False)]
            geos += [SC.cmp_mask_geometry(dtype, al, self.cus) for al in (True, False)]
            rows = SC.all_edge_rows(geos, lambda R, G, v: SC.size_list(R, G, v, seed=R + v))
            seed = 100 + SC.ALL_DTYPES.index(dtype)
            b = SC.plant(SC.uniform_column(dtype, n, seed), rows)
            a = SC.plant(SC.uniform_column(dtype, n, seed + 50), rows, shift=2)
            self._cols[key] = (b, a, self.ctx.upload(b), self.ctx.upload(a))
        return self._cols[key]

    def cond(self):
        if self._m is None:
            n = max(SC.max_rows(self.cus, d) for d in SC.ALL_DTYPES) + 4
            m = SC.mask_column(n, 77)
            self._m = (m, self.ctx.upload(m))
        return self._m

    def ref_mask(self, dtype, start, op, scalar, tag):
        """oracle mask of the pred column from row `start` on; a shorter view's mask is its prefix (the comparison is row-wise)"""
        key = (SC.name(dtype), start, op, repr(scalar), tag)
        if key not in self._masks:
            if len(self._masks) > 24:
                self._masks.clear()
            self._masks[key] = self.O.cmp_const(self.pair(dtype)[0][start:], op, scalar, tag)
        return self._masks[key]

    # -- expression columns: up to four per type, long enough for every fused-expression family
    def x_rows(self):
        worst = 0
        for d in (np.uint32, np.int64):
            R, G, v = SC.expr_same_geometry(d, self.cus)
            worst = max(worst, (2 * G + 1) * R + v + 3)
        R, G, v = SC.expr_narrow_geometry(self.cus)
        worst = max(worst, (2 * G + 1) * R + v + 3)
        R, G, v = SC.jit_sum_geometry([np.uint32], True, self.cus)
        return max(worst, (2 * G + 1) * R + v + 3) + 4

    def x_geometries(self):
        g = [SC.expr_same_geometry(d, self.cus) for d in (np.int64, np.uint32)]
        g += [SC.expr_narrow_geometry(self.cus), SC.expr_mixed_geometry(self.cus)]
        g += [SC.jit_sum_geometry([np.uint32], al, self.cus) for al in (True, False)]
        return g

    def xcol(self, dtype, k):
        key = (SC.name(dtype), k)
        if key not in self._x:
            n = self.x_rows() if np.dtype(dtype).itemsize < 8 else self.x_rows() // 2 + 8
            if not hasattr(self, "_x_edges"):
                self._x_edges = SC.all_edge_rows(self.x_geometries(), lambda R, G, v: SC.size_list(R, G, v, seed=R + v))
            c = SC.plant(SC.uniform_column(dtype, n, 500 + 10 * SC.ALL_DTYPES.index(dtype) + k), self._x_edges, shift=k)
            self._x[key] = (c, self.ctx.upload(c))
        return self._x[key]


@pytest.fixture(scope="module")
def env(oracle_mod):
    import clickhouse_amd
    e = Env(clickhouse_amd, oracle_mod)
    yield e
    e._cols.clear(), e._x.clear(), e._masks.clear()
    e._m = None
    e.ctx.close()


def bits(x) -> int:
    """the 8 bytes of a sum (Int64, UInt64 or Float64) as an integer"""
    a = np.asarray(x).reshape(1)
    assert a.dtype.itemsize == 8, a.dtype
    return int(a.view(np.uint64)[0])


def same_sum(got, want) -> bool:
    """same dtype and same bits; two NaNs count as equal whatever their payload"""
    g, w = np.asarray(got), np.asarray(want)
    if g.dtype != w.dtype:
        return False
    if g.dtype.kind == "f" and np.isnan(g) and np.isnan(w):
        return True
    return bits(g) == bits(w)


def scalars_for(dtype):
    """(scalar, tag) at the threshold: typed as the column, as the other signedness and as a fractional Float64"""
    t = SC.threshold(dtype)
    kind = np.dtype(dtype).kind
    if kind == "f":
        return [(float(t), None), (t, I64), (t + 0.5, F64)]
    out = [(t, None)]
    out.append((max(t, 0), U64) if kind == "i" else ((t, I64) if t < 2 ** 63 else (-1, I64)))
    if abs(t) < 2 ** 52:
        out.append((t + 0.5, F64))
    else:
        out.append((float(2 ** 63) if kind == "u" else -0.5, F64))
    return out


# ----------------------------------------------------------------------------------------------------------------
# 1. chgpu_filter_sum: k_filter_sum<T, VEC, SAME, false, IntRangePred | F64Pred<op>>
# ----------------------------------------------------------------------------------------------------------------
FS_LAYOUTS = [("same", "aligned"), ("same", "row1"), ("two", "aligned"), ("two", "row1"), ("two", "pred_row1"), ("two", "val_row1")]


@pytest.mark.parametrize("cols,layout", FS_LAYOUTS, ids=["-".join(x) for x in FS_LAYOUTS])
@pytest.mark.parametrize("dtype", SC.ALL_DTYPES, ids=SC.name)
def test_filter_sum_every_type_alignment_operator_and_size(env, dtype, cols, layout):
    ch, O = env.ch, env.O
    same = cols == "same"
    b, a, B, A = env.pair(dtype)
    ps = 1 if layout in ("row1", "pred_row1") else 0
    vs = ps if same else (1 if layout in ("row1", "val_row1") else 0)
    R, G, vec = SC.filter_sum_geometry(dtype, same, ps == 0 and vs == 0, env.cus)
    thr = float(SC.threshold(dtype)) if np.dtype(dtype).kind == "f" else SC.threshold(dtype)
    cases = [(SC.mid_size(R), op, s, tag) for op in ALL_OPS for s, tag in scalars_for(dtype)]
    if layout in ("aligned", "row1"):       # the half-misaligned layouts run the same VEC = 1 kernel as row1: mid-size only
        cases += [(n, op, thr, None) for n in SC.size_list(R, G, vec, seed=R + vec) for op in (LT, NE)]
    for n, op, scalar, tag in cases:
        pv = B.cut(ps, n)
        s, c = ch.filter_sum(pv, op, scalar, None if same else A.cut(vs, n), scalar_tag=tag)
        m = env.ref_mask(dtype, ps, op, scalar, tag)[:n]
        want = O.sum_add_many_conditional((b if same else a)[vs:vs + n], m)[0]
        where = (SC.name(dtype), cols, layout, SC.OP_NAMES[op], scalar, tag, n)
        assert c == O.count_bytes_in_filter(m), where
        assert same_sum(s, want), (where, s, want)


@pytest.mark.parametrize("dtype", [np.int64, np.uint8, np.int16, np.float64, np.float32], ids=SC.name)
def test_filter_sum_small_cases_agree_with_python_arithmetic(env, dtype):
    """the oracle is not the only witness: Python integers (modulo 2^64) / math.fsum over the selected rows"""
    ch = env.ch
    b, a, B, A = env.pair(dtype)
    R, G, vec = SC.filter_sum_geometry(dtype, False, True, env.cus)
    n = min(R + vec + 1, 3000)
    for start in (0, 1):
        for op in ALL_OPS:
            for s, tag in scalars_for(dtype):
                got_s, got_c = ch.filter_sum(B.cut(start, n), op, s, A.cut(start, n), scalar_tag=tag)
                want_s, want_c = SC.py_filter_sum(b[start:start + n], op, s, a[start:start + n])
                assert got_c == want_c and (float(got_s) if np.dtype(dtype).kind == "f" else int(got_s)) == want_s, (SC.name(dtype), start, op, s, tag)


def test_filter_sum_async_writes_sum_bits_and_count(env):
    ch, O = env.ch, env.O
    for dtype in (np.int64, np.float64, np.int8, np.float32):
        b, a, B, A = env.pair(dtype)
        R, G, vec = SC.filter_sum_geometry(dtype, False, True, env.cus)
        n = SC.mid_size(R) + 1
        thr = float(SC.threshold(dtype)) if np.dtype(dtype).kind == "f" else SC.threshold(dtype)
        for start in (0, 1):
            for val in (None, A):
                r = env.ctx.upload(np.full(2, 0xDEADBEEF, dtype=np.uint64))
                ch.filter_sum_async(B.cut(start, n), GE, thr, None if val is None else A.cut(start, n), r)
                env.ctx.synchronize()
                got = r.numpy()
                m = O.cmp_const(b[start:start + n], GE, thr)
                want = O.sum_add_many_conditional((b if val is None else a)[start:start + n], m)[0]
                assert int(got[1]) == O.count_bytes_in_filter(m) and int(got[0]) == bits(want), (SC.name(dtype), start, val is None)
    # predicate and value of different types: mask + conditional sum, same two words
    bp, _, BP, _ = env.pair(np.uint16)
    _, av, _, AV = env.pair(np.float64)
    n = 70_001
    r = env.ctx.upload(np.zeros(2, dtype=np.uint64))
    ch.filter_sum_async(BP.cut(0, n), LT, SC.threshold(np.uint16), AV.cut(0, n), r)
    env.ctx.synchronize()
    m = O.cmp_const(bp[:n], LT, SC.threshold(np.uint16))
    assert r.numpy().tolist() == [bits(O.sum_add_many_conditional(av[:n], m)[0]), O.count_bytes_in_filter(m)]


# ----------------------------------------------------------------------------------------------------------------
# 1b. chgpu_sum_add_many(_conditional): k_filter_sum<T, VEC, true, HAS_COND, TruePred>
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["row_begin_0", "row_begin_one_vector", "row_begin_1", "mask_view_row1"])
@pytest.mark.parametrize("dtype", SC.ALL_DTYPES, ids=SC.name)
def test_sum_add_many_with_and_without_mask_row_ranges_and_state(env, dtype, place):
    """row_begin = 16 / sizeof(T) keeps the data pointer 16-byte aligned while the mask pointer is only VEC-aligned (vector kernel);
    row_begin = 1 misaligns both, a mask view starting at row 1 misaligns the mask alone (VEC = 1 kernels)"""
    ch, O = env.ch, env.O
    _, a, _, A = env.pair(dtype)
    m, M = env.cond()
    L = a.shape[0] - 1
    rb = {"row_begin_0": 0, "row_begin_one_vector": SC.vecw(dtype), "row_begin_1": 1, "mask_view_row1": 0}[place]
    ms = 1 if place == "mask_view_row1" else 0
    col, cnd = A.cut(0, L), M.cut(ms, L)
    aligned = place in ("row_begin_0", "row_begin_one_vector")
    R, G, vec = SC.filter_sum_geometry(dtype, True, aligned, env.cus)
    rdt = O.sum_result_dtype(O.TAG_OF[np.dtype(dtype)])
    for n in SC.size_list(R, G, vec, seed=R + vec + 1):
        if rb + n > L:
            continue
        where = (SC.name(dtype), place, n)
        got = ch.sum_add_many_conditional(col, cnd, rb, rb + n)
        want = O.sum_add_many_conditional(a[rb:rb + n], m[ms + rb:ms + rb + n])
        assert same_sum(got[0], want[0]), (where, "conditional", got, want)
        if ms == 0:
            got = ch.sum_add_many(col, rb, rb + n)
            want = O.sum_add_many(a, rb, rb + n)
            assert same_sum(got[0], want[0]), (where, "plain", got, want)
    # state carried across two calls (addBatchSinglePlace twice on one place)
    n = SC.mid_size(R)
    h = n // 2 + 1
    st, so = np.array([123], dtype=rdt), np.array([123], dtype=rdt)
    ch.sum_add_many_conditional(col, cnd, rb, rb + h, st)
    ch.sum_add_many_conditional(col, cnd, rb + h, rb + n, st)
    O.sum_add_many_conditional(a[rb:rb + h], m[ms + rb:ms + rb + h], so)
    O.sum_add_many_conditional(a[rb + h:rb + n], m[ms + rb + h:ms + rb + n], so)
    assert same_sum(st[0], so[0]), (SC.name(dtype), place, "state, conditional", st, so)
    st, so = np.array([7], dtype=rdt), np.array([7], dtype=rdt)
    ch.sum_add_many(col, rb, rb + h, st)
    ch.sum_add_many(col, rb + h, rb + n, st)
    O.sum_add_many(a, rb, rb + h, so)
    O.sum_add_many(a, rb + h, rb + n, so)
    assert same_sum(st[0], so[0]), (SC.name(dtype), place, "state, plain", st, so)


# ----------------------------------------------------------------------------------------------------------------
# 1c. predicate and value of different types: k_cmp_mask, then k_filter_sum<T, VEC, true, true, TruePred>
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", SC.ALL_DTYPES, ids=SC.name)
def test_filter_sum_predicate_of_another_type(env, vdtype):
    ch, O = env.ch, env.O
    _, a, _, A = env.pair(vdtype)
    for pdtype in (np.uint8, np.int16, np.uint32, np.int64, np.float64):       # 1, 2, 4, 8 bytes and a float predicate
        if np.dtype(pdtype) == np.dtype(vdtype):
            pdtype = {np.dtype(np.uint8): np.int8, np.dtype(np.int16): np.uint16, np.dtype(np.uint32): np.int32, np.dtype(np.int64): np.uint64,
                      np.dtype(np.float64): np.float32}[np.dtype(pdtype)]
        b, _, B, _ = env.pair(pdtype)
        R, G, vec = SC.cmp_mask_geometry(pdtype, True, env.cus)
        limit = min(a.shape[0], b.shape[0]) - 1
        for n in (0, 1, vec + 1, R + vec + 1, min(SC.mid_size(R), limit)):
            for start in (0, 1):
                for op, (s, tag) in ((LT, scalars_for(pdtype)[0]), (NE, scalars_for(pdtype)[0]), (GE, scalars_for(pdtype)[2])):
                    got_s, got_c = ch.filter_sum(B.cut(start, n), op, s, A.cut(start, n), scalar_tag=tag)
                    mask = O.cmp_const(b[start:start + n], op, s, tag)
                    want = O.sum_add_many_conditional(a[start:start + n], mask)[0]
                    where = (SC.name(vdtype), SC.name(pdtype), start, SC.OP_NAMES[op], s, n)
                    assert got_c == O.count_bytes_in_filter(mask), where
                    assert same_sum(got_s, want), (where, got_s, want)


# ----------------------------------------------------------------------------------------------------------------
# 2. chgpu_cmp_const: k_cmp_mask<T, VEC, IntRangePred | F64Pred<op>>, mask bytes
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["aligned", "row1"])
@pytest.mark.parametrize("dtype", SC.ALL_DTYPES, ids=SC.name)
def test_cmp_const_mask_bytes_every_type_alignment_operator_and_size(env, dtype, layout):
    """all six operators up to a few chunks (main loop, remainder loop and scalar tail all run); `<` and `!=` up to twice the grid"""
    ch = env.ch
    b, _, B, _ = env.pair(dtype)
    start = 0 if layout == "aligned" else 1
    R, G, vec = SC.cmp_mask_geometry(dtype, start == 0, env.cus)
    thr = float(SC.threshold(dtype)) if np.dtype(dtype).kind == "f" else SC.threshold(dtype)
    for n in SC.size_list(R, G, vec, seed=R + vec + 2):
        for op in (ALL_OPS if n <= 4 * R else (LT, NE)):
            got = ch.cmp_const(B.cut(start, n), op, thr).numpy()
            want = env.ref_mask(dtype, start, op, thr, None)[:n]
            where = (SC.name(dtype), layout, SC.OP_NAMES[op], n)
            assert got.dtype == np.uint8 and got.shape == (n,), where
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError((where, "first wrong rows", bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist()))
            assert n == 0 or int(got.max()) <= 1, where
    n = SC.mid_size(R)
    for s, tag in scalars_for(dtype)[1:]:
        for op in ALL_OPS:
            got = ch.cmp_const(B.cut(start, n), op, s, tag).numpy()
            assert np.array_equal(got, env.ref_mask(dtype, start, op, s, tag)[:n]), (SC.name(dtype), layout, SC.OP_NAMES[op], s, tag, n)


# ----------------------------------------------------------------------------------------------------------------
# floats: the rounding path and the IEEE specials
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", ["same", "two"])
@pytest.mark.parametrize("dtype", SC.FLOAT_DTYPES, ids=SC.name)
def test_float_sums_of_general_values_within_1e6_of_fsum_and_reproducible(env, dtype, cols):
    """reference: math.fsum over the selected rows widened to double; bound 1e-6 * sum |x| over the selected rows (the tolerance of
    sum(Float64), applied to sum |x| so that cancellation cannot make it vacuous); three runs give identical bits"""
    ch, O = env.ch, env.O
    same = cols == "same"
    R, G, vec = SC.filter_sum_geometry(dtype, same, True, env.cus)
    N = (2 * G + 1) * R + vec + 4
    p = SC.rough_float_column(dtype, N, 31)
    v = p if same else SC.rough_float_column(dtype, N, 32)
    P = env.ctx.upload(p)
    V = P if same else env.ctx.upload(v)
    for start in (0, 1):
        for n in (1, R + vec + 1, SC.mid_size(R), N - 1):
            for op, s in ((LT, 0.25), (NE, float(p[start])), (GE, -1000.0)):
                pv = P.cut(start, n)
                runs = [ch.filter_sum(pv, op, s, None if same else V.cut(start, n), scalar_tag=F64) for _ in range(3)]
                keep = O.cmp_const(p[start:start + n], op, s, F64) != 0
                sel = v[start:start + n][keep].astype(np.float64)
                want, bound = math.fsum(sel.tolist()), 1e-6 * math.fsum(np.abs(sel).tolist())
                where = (SC.name(dtype), cols, start, SC.OP_NAMES[op], n)
                assert runs[0][1] == int(keep.sum()), where
                assert runs[0][0].dtype == np.float64 and abs(float(runs[0][0]) - want) <= bound, (where, float(runs[0][0]), want, bound)
                assert len({bits(r[0]) for r in runs}) == 1 and len({r[1] for r in runs}) == 1, where
    m = SC.mask_column(N, 33)
    M = env.ctx.upload(m)
    for start in (0, 1):
        n = N - 1
        runs = [ch.sum_add_many_conditional(P.cut(start, n), M.cut(start, n))[0] for _ in range(3)]
        sel = p[start:start + n][m[start:start + n] != 0].astype(np.float64)
        assert abs(float(runs[0]) - math.fsum(sel.tolist())) <= 1e-6 * math.fsum(np.abs(sel).tolist()) and len({bits(r) for r in runs}) == 1, (SC.name(dtype), start)


def _special_columns(dtype, env):
    """name -> (pred, val): n = one chunk + one vector + 1 rows, the special planted in the main loop, the remainder and the tail"""
    R, G, vec = SC.filter_sum_geometry(dtype, False, True, env.cus)
    n = R + vec + 1
    rng = np.random.Generator(np.random.PCG64(41))
    base = rng.integers(-100, 100, size=n).astype(dtype)
    spots = [0, R - 1, R, n - 1]

    def with_(vals):
        c = base.copy()
        for k, r in enumerate(spots):
            c[r] = vals[k % len(vals)]
        return c
    ones = np.ones(n, dtype=dtype)
    return {
        "nan_in_predicate": (with_([np.nan]), ones),
        "selected_plus_inf": (base, with_([np.inf])),
        "plus_and_minus_inf": (base, with_([np.inf, -np.inf])),
        "selected_nan": (base, with_([np.nan])),
        "only_minus_zero": (np.full(n, -0.0, dtype=dtype), np.full(n, -0.0, dtype=dtype)),
    }


@pytest.mark.parametrize("case", ["nan_in_predicate", "selected_plus_inf", "plus_and_minus_inf", "selected_nan", "only_minus_zero"])
@pytest.mark.parametrize("dtype", SC.FLOAT_DTYPES, ids=SC.name)
def test_float_specials_follow_ieee_like_the_oracle(env, dtype, case):
    ch, O = env.ch, env.O
    p, v = _special_columns(dtype, env)[case]
    n = p.shape[0] - 1
    P, V = env.ctx.upload(p), env.ctx.upload(v)
    for start in (0, 1):
        for s in (0.0, float("nan"), -0.0, 50.0):
            for op in ALL_OPS:
                where = (SC.name(dtype), case, start, SC.OP_NAMES[op], s)
                mask = O.cmp_const(p[start:start + n], op, s, F64)
                assert np.array_equal(ch.cmp_const(P.cut(start, n), op, s, F64).numpy(), mask), where
                for two in (False, True):
                    val = v if two else p
                    got_s, got_c = ch.filter_sum(P.cut(start, n), op, s, V.cut(start, n) if two else None, scalar_tag=F64)
                    want = O.sum_add_many_conditional(val[start:start + n], mask)[0]
                    assert got_c == O.count_bytes_in_filter(mask), (where, two)
                    assert same_sum(got_s, want), (where, two, got_s, want)
        # no predicate at all: sum of the column, with and without a mask
        cond = SC.mask_column(n, 43, keep_one_in=2)
        assert same_sum(ch.sum_add_many(V.cut(start, n))[0], O.sum_add_many(v, start, start + n)[0]), (SC.name(dtype), case, start)
        assert same_sum(ch.sum_add_many_conditional(V.cut(start, n), env.ctx.upload(cond))[0], O.sum_add_many_conditional(v[start:start + n], cond)[0]), (SC.name(dtype), case, start)


def test_float32_column_against_a_float64_constant_float32_cannot_represent(env):
    """0.1 is not a Float32: the column is widened exactly and compared in double, so `=` selects nothing even where the column holds
    Float32(0.1), and `<` / `>` split on the double"""
    ch, O = env.ch, env.O
    R, G, vec = SC.filter_sum_geometry(np.float32, True, True, env.cus)
    n = R + vec + 1
    rng = np.random.Generator(np.random.PCG64(45))
    p = rng.choice(np.array([0.1, 0.25, -0.1, 0.0, 0.100000024, 0.099999994, 1.0], dtype=np.float32), size=n + 1)
    P = env.ctx.upload(p)
    for start in (0, 1):
        for s in (0.1, float(np.float32(0.1))):
            for op in ALL_OPS:
                mask = O.cmp_const(p[start:start + n], op, s, F64)
                assert np.array_equal(ch.cmp_const(P.cut(start, n), op, s, F64).numpy(), mask), (start, s, op)
                got_s, got_c = ch.filter_sum(P.cut(start, n), op, s, scalar_tag=F64)
                assert got_c == O.count_bytes_in_filter(mask) == sum(SC.py_pass(p[start:start + n], op, s)), (start, s, op)
                want = math.fsum(p[start:start + n][mask != 0].astype(np.float64).tolist())
                assert abs(float(got_s) - want) <= 1e-6 * abs(want) + 1e-12, (start, s, op)
        assert ch.filter_sum(P.cut(start, n), EQ, 0.1, scalar_tag=F64)[1] == 0
        assert ch.filter_sum(P.cut(start, n), EQ, float(np.float32(0.1)), scalar_tag=F64)[1] == int((p[start:start + n] == np.float32(0.1)).sum()) > 0


# ----------------------------------------------------------------------------------------------------------------
# 3. chgpu_expr_filter_sum: k_expr_filter_sum<T>, k_expr_filter_sum_narrow<WMASK>, k_expr_filter_sum_mixed
# ----------------------------------------------------------------------------------------------------------------
def std_preds(dtypes):
    """three predicates spread over the columns (on one column when there is only one): < about the median, != a planted value,
    >= the first quarter of the range"""
    k = len(dtypes)
    out = [(0, LT, SC.threshold(dtypes[0]))]
    c = 1 % k
    out.append((c, NE, SC.threshold(dtypes[c]) + 1))
    c = 2 % k
    lo, hi = SC.limits(dtypes[c])
    out.append((c, GE, lo + (hi - lo) // 4))
    return out


def check_expr(env, dtypes, picks, n, preds, vop, va, vb, where):
    """device == oracle (sum bits, dtype, count); Python integers as well where the case is small"""
    ch, O = env.ch, env.O
    pairs = [env.xcol(d, k) for d, k in zip(dtypes, picks)]
    host = [p[0][:n] for p in pairs]
    dev = [p[1].cut(0, n) for p in pairs]
    s, c = ch.expr_filter_sum(dev, preds, vop, va, vb)
    so, co = O.expr_filter_sum_pipeline(host, preds, vop, va, vb)
    assert s.dtype == so.dtype and (bits(s), c) == (bits(so), co), (where, (s, c), (so, co))
    if n <= 5000:
        ps, pc, signed = SC.py_expr_filter_sum(host, preds, vop, va, vb)
        assert (int(s), c) == (ps, pc) and (s.dtype == np.int64) == signed, (where, "python", (s, c), (ps, pc))
    return s, c


VALUE_FORMS = [(SC.VAL_MUL, -1, 0), (SC.VAL_COL, -1, 0), (SC.VAL_PLUS, 0, -1), (SC.VAL_MINUS, -1, 0), (SC.VAL_MUL, 0, 0)]


def value_form(i, n_cols):
    vop, va, vb = VALUE_FORMS[i % len(VALUE_FORMS)]
    return vop, va % n_cols, vb % n_cols


@pytest.mark.parametrize("n_cols", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [np.int64, np.uint64, np.uint32, np.int32], ids=SC.name)
def test_expr_same_type_kernel_every_column_count_and_size(env, dtype, n_cols):
    dtypes = [dtype] * n_cols
    R, G, vec = SC.expr_same_geometry(dtype, env.cus)
    preds = std_preds(dtypes)
    for i, n in enumerate(SC.size_list(R, G, vec, seed=R + vec + 3)):
        vop, va, vb = value_form(i, n_cols)
        check_expr(env, dtypes, range(n_cols), n, preds, vop, va, vb, (SC.name(dtype), n_cols, n, SC.VAL_NAMES[vop], va, vb))
    for i in range(len(VALUE_FORMS)):
        vop, va, vb = value_form(i, n_cols)
        for n in (R + vec + 1, SC.mid_size(R)):
            check_expr(env, dtypes, range(n_cols), n, preds, vop, va, vb, (SC.name(dtype), n_cols, n, SC.VAL_NAMES[vop], va, vb))


def narrow_types(wmask):
    """bit k set: column k is 4 bytes wide, UInt32 and Int32 in turn (so WMASK = 15 is not one type); else UInt8"""
    return [(np.uint32, np.int32)[k % 2] if (wmask >> k) & 1 else np.uint8 for k in range(4)]


@pytest.mark.parametrize("wmask", range(16))
def test_expr_narrow_kernel_every_width_mask_and_size(env, wmask):
    dtypes = narrow_types(wmask)
    R, G, vec = SC.expr_narrow_geometry(env.cus)
    preds = std_preds(dtypes) + [(3, LE, SC.limits(dtypes[3])[1] - 3)]
    for i, n in enumerate(SC.size_list(R, G, vec, seed=wmask)):
        vop, va, vb = value_form(i + wmask, 4)
        check_expr(env, dtypes, range(4), n, preds, vop, va, vb, ("wmask", wmask, n, SC.VAL_NAMES[vop], va, vb))
    for i in range(len(VALUE_FORMS)):
        vop, va, vb = value_form(i, 4)
        check_expr(env, dtypes, range(4), R + vec + 1, preds, vop, va, vb, ("wmask", wmask, R + vec + 1, SC.VAL_NAMES[vop], va, vb))


NARROW_FEWER = [[np.uint8], [np.uint8, np.uint32], [np.uint32, np.uint8], [np.int32, np.uint32], [np.uint8, np.uint8, np.int32],
                [np.uint32, np.uint8, np.int32], [np.int32, np.uint8, np.uint8], [np.uint8, np.uint8]]


@pytest.mark.parametrize("dtypes", NARROW_FEWER, ids=["+".join(SC.name(d) for d in t) for t in NARROW_FEWER])
def test_expr_narrow_kernel_fewer_than_four_columns(env, dtypes):
    """the absent columns alias column 0, which also decides their bit of WMASK"""
    R, G, vec = SC.expr_narrow_geometry(env.cus)
    k = len(dtypes)
    for i, n in enumerate((0, 1, vec + 1, R - 1, R + vec + 1, SC.mid_size(R), G * R + 1)):
        vop, va, vb = value_form(i, k)
        check_expr(env, dtypes, range(k), n, std_preds(dtypes), vop, va, vb, ([SC.name(d) for d in dtypes], n, SC.VAL_NAMES[vop], va, vb))


MIXED = [[np.int64, np.uint8, np.uint32, np.int32], [np.uint8, np.uint64, np.int32, np.uint32], [np.uint32, np.int32, np.int64, np.uint8],
         [np.int32, np.uint8, np.uint32, np.uint64], [np.uint8, np.int64], [np.uint64, np.int32, np.uint8], [np.int64, np.uint64, np.uint32]]


@pytest.mark.parametrize("dtypes", MIXED, ids=["+".join(SC.name(d) for d in t) for t in MIXED])
def test_expr_mixed_kernel_eight_byte_column_in_every_position(env, dtypes):
    R, G, vec = SC.expr_mixed_geometry(env.cus)
    k = len(dtypes)
    sizes = SC.size_list(R, G, vec, seed=k) + [4 * G * R - 1, 4 * G * R, 4 * G * R + 1, 9 * G * R + 7]   # 4 steps in flight, a grid apart
    for i, n in enumerate(sizes):
        vop, va, vb = value_form(i, k)
        check_expr(env, dtypes, range(k), n, std_preds(dtypes), vop, va, vb, ([SC.name(d) for d in dtypes], n, SC.VAL_NAMES[vop], va, vb))
    for i in range(len(VALUE_FORMS)):
        vop, va, vb = value_form(i, k)
        check_expr(env, dtypes, range(k), 4 * R + 3, std_preds(dtypes), vop, va, vb, ([SC.name(d) for d in dtypes], 4 * R + 3, SC.VAL_NAMES[vop], va, vb))


FAMILIES = {"same": [np.uint32] * 4, "same64": [np.int64] * 4, "narrow": [np.uint32, np.uint8, np.uint8, np.int32], "mixed": [np.int32, np.int64, np.uint64, np.uint8]}


def _inner_range(dtype):
    lo, hi = SC.limits(dtype)
    return lo + (hi - lo) // 8, hi - (hi - lo) // 8


@pytest.mark.parametrize("family", list(FAMILIES))
def test_expr_predicate_counts_and_placement(env, family):
    """0, 1 and 8 predicates; three on one column; predicates on the value columns; columns that only carry the value"""
    dtypes = FAMILIES[family]
    R = {"same": SC.expr_same_geometry(np.uint32, env.cus), "same64": SC.expr_same_geometry(np.int64, env.cus), "narrow": SC.expr_narrow_geometry(env.cus),
         "mixed": SC.expr_mixed_geometry(env.cus)}[family][0]
    q = [_inner_range(d) for d in dtypes]
    t = [SC.threshold(d) for d in dtypes]
    sets = {
        "none": [],
        "one": [(2, GT, t[2])],
        "eight": [(k, GE, q[k][0]) for k in range(4)] + [(k, LE, q[k][1]) for k in range(4)],
        "three_on_one_column": [(1, GE, q[1][0]), (1, LE, q[1][1]), (1, NE, t[1])],
        "on_the_value_columns": [(3, LT, t[3]), (0, GE, q[0][0])],
        "value_columns_carry_no_predicate": [(1, LT, t[1]), (2, NE, t[2] - 1)],
    }
    for label, preds in sets.items():
        for n in (R + 5, SC.mid_size(R), 4999):
            for vop, va, vb in ((SC.VAL_MUL, 3, 0), (SC.VAL_COL, 3, 0), (SC.VAL_MINUS, 0, 3)):
                check_expr(env, dtypes, range(4), n, preds, vop, va, vb, (family, label, n, SC.VAL_NAMES[vop]))


FOLD = [(np.uint8, "narrow"), (np.uint8, "mixed"), (np.uint32, "same"), (np.uint32, "narrow"), (np.uint32, "mixed"), (np.int32, "same"), (np.int32, "narrow"),
        (np.int32, "mixed"), (np.int64, "same"), (np.int64, "mixed"), (np.uint64, "same"), (np.uint64, "mixed")]


@pytest.mark.parametrize("dtype,family", FOLD, ids=[SC.name(d) + "-" + f for d, f in FOLD])
def test_expr_constant_fold_inside_at_and_outside_the_column_range(env, dtype, family):
    """every operator against constants inside the column's range, at its ends and outside on both sides, typed as the column, as Int64
    (negative against unsigned), as UInt64 (>= 2^63 against signed) and as a fractional Float64: `=` / `<` against an impossible
    constant select nothing, `!=` / `>=` everything.  Count and sum against Python integers and against the oracle."""
    ch, O = env.ch, env.O
    other = {"same": dtype, "narrow": np.uint8 if np.dtype(dtype).itemsize == 4 else np.uint32, "mixed": np.int64 if np.dtype(dtype) != np.dtype(np.int64) else np.uint8}[family]
    dtypes = [other, dtype]
    n = 2 * 2048 + 7
    pairs = [env.xcol(d, k) for k, d in enumerate(dtypes)]
    host = [p[0][:n] for p in pairs]
    dev = [p[1].cut(0, n) for p in pairs]
    tag_of = {np.dtype(np.int64): I64, np.dtype(np.uint64): U64, np.dtype(np.float64): F64}
    col = host[1].tolist()
    for scalar, sdt in SC.fold_constants(dtype):
        tag = None if np.dtype(sdt) == np.dtype(dtype) else tag_of[np.dtype(sdt)]
        for op in ALL_OPS:
            preds = [(1, op, scalar, tag)]
            s, c = ch.expr_filter_sum(dev, preds, SC.VAL_COL, 1)
            keep = [SC.OPS[op](x, scalar) for x in col]
            want = SC.wrap64(sum(x for x, k in zip(col, keep) if k), np.dtype(dtype).kind == "i")
            where = (SC.name(dtype), family, SC.OP_NAMES[op], scalar, SC.name(sdt))
            assert (int(s), c) == (want, sum(keep)), (where, (int(s), c), (want, sum(keep)))
            so, co = O.expr_filter_sum_pipeline(host, preds, SC.VAL_COL, 1)
            assert s.dtype == so.dtype and (bits(s), c) == (bits(so), co), (where, "oracle")
            lo, hi = SC.limits(dtype)
            if scalar > hi or scalar < lo:      # impossible constant: nothing or everything
                assert c == (n if op == NE or (op in (LT, LE) and scalar > hi) or (op in (GT, GE) and scalar < lo) else 0), where


PAIRS = [(a, b) for a in SC.EXPR_DTYPES for b in SC.EXPR_DTYPES]


@pytest.mark.parametrize("ta,tb", PAIRS, ids=[SC.name(a) + "-" + SC.name(b) for a, b in PAIRS])
def test_expr_value_operators_over_every_operand_type_pair(env, ta, tb):
    """multiply / plus / minus / a bare column over every ordered pair of operand types; columns are uniform over their whole range, so
    Int64 x Int64, UInt64 - UInt64 and UInt32 x UInt32 (above 2^63) wrap; result dtype against cho_arith_sum_type"""
    O = env.O
    dtypes = [ta, tb]
    n = 4101
    for vop in (SC.VAL_COL, SC.VAL_MUL, SC.VAL_PLUS, SC.VAL_MINUS):
        for va, vb in ((0, 1), (1, 0), (0, 0)):
            s, c = check_expr(env, dtypes, (0, 1), n, [(1, NE, SC.threshold(tb))], vop, va, vb, (SC.name(ta), SC.name(tb), SC.VAL_NAMES[vop], va, vb))
            x, y = dtypes[va], dtypes[vb if vop != SC.VAL_COL else va]
            rt = O.sum_result_dtype(O.TAG_OF[np.dtype(x)]) if vop == SC.VAL_COL else O.NP_OF[O.lib().cho_arith_sum_type(vop, O.TAG_OF[np.dtype(x)], O.TAG_OF[np.dtype(y)])]
            assert s.dtype == np.dtype(rt), (SC.name(ta), SC.name(tb), SC.VAL_NAMES[vop], va, vb, s.dtype, rt)
    # the wrap-around really happens in these columns
    a, b = env.xcol(ta, 0)[0][:n].tolist(), env.xcol(tb, 1)[0][:n].tolist()
    if np.dtype(ta).itemsize == 8 and np.dtype(tb).itemsize == 8:
        assert any(abs(x * y) >= 2 ** 64 for x, y in zip(a, b))
    if np.dtype(ta) == np.dtype(tb) == np.dtype(np.uint32):
        assert any(x * y >= 2 ** 63 for x, y in zip(a, b))


def test_expr_errors_leave_the_context_usable(env):
    ch = env.ch
    K = ch._capi
    n = 4096
    u32 = [env.xcol(np.uint32, k)[1].cut(0, n) for k in range(4)]

    def code(f):
        with pytest.raises(ch.ChgpuError) as e:
            f()
        return e.value.code
    assert code(lambda: ch.expr_filter_sum(u32 + [u32[0]], [], SC.VAL_COL, 0)) == K.ERR_NOT_IMPLEMENTED            # five columns
    assert code(lambda: ch.expr_filter_sum(u32, [(0, LT, 5)] * 9, SC.VAL_COL, 0)) == K.ERR_NOT_IMPLEMENTED         # nine predicates
    f64 = env.pair(np.float64)[3].cut(0, n)
    u16 = env.pair(np.uint16)[3].cut(0, n)
    assert code(lambda: ch.expr_filter_sum([u32[0], f64], [], SC.VAL_COL, 0)) == K.ERR_NOT_IMPLEMENTED
    assert code(lambda: ch.expr_filter_sum([u16, u32[0]], [], SC.VAL_COL, 1)) == K.ERR_NOT_IMPLEMENTED
    assert code(lambda: ch.expr_filter_sum([u32[0], u32[1].cut(0, n - 1)], [], SC.VAL_COL, 0)) == K.ERR_SIZES_MISMATCH
    assert code(lambda: ch.expr_filter_sum(u32[:2], [], SC.VAL_COL, 2)) == K.ERR_BAD_ARGUMENTS
    assert code(lambda: ch.expr_filter_sum(u32[:2], [], SC.VAL_MUL, 0, 2)) == K.ERR_BAD_ARGUMENTS
    assert code(lambda: ch.expr_filter_sum(u32[:2], [(2, LT, 5, U32)], SC.VAL_COL, 0)) == K.ERR_BAD_ARGUMENTS
    full = [env.xcol(np.uint32, k)[1] for k in range(2)]
    assert code(lambda: ch.expr_filter_sum([c.cut(1, n) for c in full], [], SC.VAL_COL, 0)) == K.ERR_NOT_IMPLEMENTED   # not 16-byte aligned
    check_expr(env, [np.uint32] * 4, range(4), n, std_preds([np.uint32] * 4), SC.VAL_MUL, 3, 1, "good call after the errors")


# ----------------------------------------------------------------------------------------------------------------
# 4. the generated kernel: the same cases as a DAG through ExpressionActions.filter_sum
# ----------------------------------------------------------------------------------------------------------------
CMP_NAMES = {EQ: "equals", NE: "notEquals", LT: "less", GT: "greater", LE: "lessOrEquals", GE: "greaterOrEquals"}
VAL_FUNCS = {SC.VAL_MUL: "multiply", SC.VAL_PLUS: "plus", SC.VAL_MINUS: "minus"}


def dag_of(ch, dtypes, preds, vop, va, vb):
    d = ch.ActionsDAG()
    ins = [d.add_input(j, dt) for j, dt in enumerate(dtypes)]
    f = None
    for ci, op, sc in preds:
        node = d.add_function(CMP_NAMES[op], ins[ci], d.add_column(sc, dtypes[ci]))
        f = node if f is None else d.add_function("and", f, node)
    v = ins[va] if vop == SC.VAL_COL else d.add_function(VAL_FUNCS[vop], ins[va], ins[vb])
    return d.compile(), (-1 if f is None else f), v


JIT_CASES = {
    "q11_uint32": ([np.uint32] * 4, SC.VAL_MUL, 3, 1),
    "ssb_widths": ([np.uint32, np.uint8, np.uint8, np.uint32], SC.VAL_MUL, 3, 1),
    "signed_mix": ([np.int32, np.uint8, np.uint32, np.int32], SC.VAL_MINUS, 0, 2),
    "int64": ([np.int64, np.int64, np.uint64], SC.VAL_MUL, 0, 1),
    "bare_column": ([np.uint8, np.int32], SC.VAL_COL, 1, 0),
}


@pytest.mark.parametrize("layout", ["aligned", "row1"])
@pytest.mark.parametrize("case", list(JIT_CASES))
def test_generated_kernel_equals_hand_fused_kernel_and_oracle(env, case, layout):
    """three implementations, one answer: the run-time compiled k_run, the hand-fused entry point and the CPU oracle"""
    ch, O = env.ch, env.O
    dtypes, vop, va, vb = JIT_CASES[case]
    preds = std_preds(dtypes)
    ex, f, v = dag_of(ch, dtypes, preds, vop, va, vb)
    start = 0 if layout == "aligned" else 1
    R, G, vec = SC.jit_sum_geometry(dtypes, start == 0, env.cus)
    pairs = [env.xcol(d, k) for k, d in enumerate(dtypes)]
    for n in SC.size_list(R, G, vec, seed=R + vec + 4):
        host = [p[0][start:start + n] for p in pairs]
        dev = [p[1].cut(start, n) for p in pairs]
        where = (case, layout, n)
        s, c = ex.filter_sum(env.ctx, dev, f, v)
        so, co = O.expr_filter_sum_pipeline(host, preds, vop, va, vb)
        assert s.dtype == so.dtype and (bits(s), c) == (bits(so), co), (where, (s, c), (so, co))
        if start == 0 or n <= 4 * R:
            fused = dev if start == 0 else [env.ctx.upload(h) for h in host]   # the hand-fused kernels want 16-byte aligned columns
            s2, c2 = ch.expr_filter_sum(fused, preds, vop, va, vb)
            assert s2.dtype == s.dtype and (bits(s2), c2) == (bits(s), c), (where, "hand-fused", (s2, c2), (s, c))
        if n in (R + 1, G * R + 1):
            s0, c0 = ex.filter_sum(env.ctx, dev, f, -1)                        # count only
            assert c0 == co and int(s0) == 0, (where, "count only")
            assert ex.filter_sum(env.ctx, dev, -1, -1)[1] == n, (where, "count only, no WHERE")


@pytest.mark.parametrize("layout", ["aligned", "row1"])
@pytest.mark.parametrize("dtype", SC.FLOAT_DTYPES, ids=SC.name)
def test_generated_kernel_float_value_node_is_bit_exact_on_exactly_summable_input(env, dtype, layout):
    ch, O = env.ch, env.O
    d = ch.ActionsDAG()
    key, x, y = d.add_input(0, np.uint32), d.add_input(1, dtype), d.add_input(2, dtype)
    thr = SC.threshold(np.uint32)
    f = d.add_function("less", key, d.add_column(thr, np.uint32))
    v = d.add_function("plus", x, y)
    ex = d.compile()
    assert ex.node_dtype(v).kind == "f"
    kh, K = env.xcol(np.uint32, 0)
    b, a, B, A = env.pair(dtype)
    start = 0 if layout == "aligned" else 1
    R, G, vec = SC.jit_sum_geometry([np.uint32, dtype, dtype], start == 0, env.cus)
    for n in SC.size_list(R, G, vec, seed=R + vec + 5):
        if start + n > min(b.shape[0], kh.shape[0]):
            continue
        s, c = ex.filter_sum(env.ctx, [K.cut(start, n), B.cut(start, n), A.cut(start, n)], f, v)
        mask = O.cmp_const(kh[start:start + n], LT, thr)
        total = (b[start:start + n].astype(np.float64) + a[start:start + n].astype(np.float64))      # |x + y| <= 2^21: exact in either float type
        want = O.sum_add_many_conditional(total, mask)[0]
        where = (SC.name(dtype), layout, n)
        assert c == O.count_bytes_in_filter(mask), where
        assert same_sum(s, want) and float(s) == math.fsum(total[mask != 0].tolist()), (where, s, want)
