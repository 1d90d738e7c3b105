"""The case generators and references of tests/test_gpu_streaming_matrix.py, checked without a device: the oracle expectation of
every case family equals an independent Python / numpy computation at a small size, the exactly summable float columns really are,
and the size lists straddle every kernel's chunk and grid for a 256-CU device."""
import math
import os
import re

import numpy as np
import pytest

import streaming_cases as SC

CUS = 256
EQ, NE, LT, GT, LE, GE = range(6)
I64, U32, U64, F64 = 0, 1, 2, 3
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "clickhouse_amd", "csrc")


def _all_geometries():
    out = {}
    for d in SC.ALL_DTYPES:
        for same in (True, False):
            for al in (True, False):
                out[("k_filter_sum", SC.name(d), same, al)] = SC.filter_sum_geometry(d, same, al, CUS)
        for al in (True, False):
            out[("k_cmp_mask", SC.name(d), al)] = SC.cmp_mask_geometry(d, al, CUS)
    for d in (np.int64, np.uint64, np.uint32, np.int32):
        out[("k_expr_filter_sum", SC.name(d))] = SC.expr_same_geometry(d, CUS)
    out[("k_expr_filter_sum_narrow",)] = SC.expr_narrow_geometry(CUS)
    out[("k_expr_filter_sum_mixed",)] = SC.expr_mixed_geometry(CUS)
    for types in ([np.uint32] * 4, [np.uint32, np.uint8], [np.int64, np.uint64], [np.uint32, np.float64, np.float64], [np.uint32, np.float32]):
        for al in (True, False):
            out[("k_run", tuple(SC.name(t) for t in types), al)] = SC.jit_sum_geometry(types, al, CUS)
    return out


def test_size_lists_straddle_chunk_and_grid_of_every_kernel():
    for key, (R, G, vec) in _all_geometries().items():
        sizes = SC.size_list(R, G, vec, seed=1)
        assert sizes == sorted(set(sizes)) and sizes[0] == 0 and 1 in sizes, key
        for edge in (vec, R, G * R):
            assert edge in sizes and (edge + 1 in sizes), (key, edge)
            assert any(s < edge for s in sizes if s > 0) or edge == 1, (key, edge)
        assert R - 1 in sizes and any((G - 1) * R < s < G * R for s in sizes), key
        assert max(sizes) > 2 * G * R and max(sizes) % vec != 0 or vec == 1, key
        assert any(s % R not in (0, 1, R - 1) and s > R for s in sizes), key     # ragged ones
        # main loop, remainder loop and scalar tail are all non-empty for the largest size
        n = max(sizes)
        rows = SC.edge_rows(n, R, vec)
        assert rows[0] == 0 and rows[-1] == n - 1 and (n // R) * R - 1 in rows and (n // R) * R in rows, key
    assert SC.max_rows(CUS, np.int8) <= 17_000_000 and SC.max_rows(CUS, np.float32) <= SC.FLOAT_EXACT_MAX_ROWS


def test_geometry_table_matches_the_constants_in_the_source():
    """the few literals R and G are derived from; a tuning change that moves them must move streaming_cases too"""
    with open(os.path.join(CSRC, "filter_kernels.hip")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "expr_jit.hip")) as f:
        jit = f.read()
    def one(pattern, text=src):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    assert one(r"FS_THREADS = (\d+);") == SC.THREADS
    assert one(r"FS_WG_PER_CU = (\d+);") == 2 and one(r"#define FS_UNROLL_SAME (\d+)") == 4
    assert one(r'"tune_cmp_wg", (\d+)\)') == 2 and one(r'"tune_expr_wg", (\d+)\)') == 3 and one(r'"tune_exprn_wg", (\d+)\)') == 6
    assert one(r"#define EX_UNROLL (\d+)") == 4 and one(r"#define EXN_UNROLL (\d+)") == 2 and one(r"#define EXM_UNROLL (\d+)") == 4
    assert one(r'"tune_jit_unroll", (\d+)\)', jit) == 4 and one(r'"tune_jit_wg_sum", (\d+)\)', jit) == 2
    assert SC.filter_sum_geometry(np.int64, True, True, CUS) == (2048, 512, 2) and SC.filter_sum_geometry(np.int8, False, True, CUS) == (8192, 512, 16)
    assert SC.filter_sum_geometry(np.uint16, True, False, CUS) == (1024, 512, 1) and SC.cmp_mask_geometry(np.uint16, True, CUS) == (8192, 512, 8)
    assert SC.cmp_mask_geometry(np.uint8, True, CUS)[0] == 16384 and SC.expr_narrow_geometry(CUS) == (2048, 1536, 4)
    assert SC.jit_sum_geometry([np.uint32, np.uint8], True, CUS) == (4096, 512, 4) and SC.jit_sum_geometry([np.uint32, np.float64], True, CUS)[2] == 2


@pytest.mark.parametrize("dtype", SC.FLOAT_DTYPES, ids=SC.name)
def test_exactly_summable_float_columns_stay_below_2_pow_53(oracle_mod, dtype):
    """integer-valued, |x| <= 2^20, at most 2^25 rows: sum |x| < 2^53, so every partial sum in any order is an exact double"""
    assert SC.FLOAT_EXACT_MAX * SC.FLOAT_EXACT_MAX_ROWS < 2 ** 53
    n = SC.max_rows(CUS, dtype)
    assert n <= SC.FLOAT_EXACT_MAX_ROWS
    col = SC.plant(SC.uniform_column(dtype, n, 3), range(0, n, 4097))
    as_int = col.astype(np.int64)
    assert np.array_equal(as_int.astype(dtype), col) and int(np.abs(as_int).max()) == SC.FLOAT_EXACT_MAX
    assert int(np.abs(as_int).sum()) < 2 ** 53
    mask = SC.mask_column(n, 5)
    exact = int(as_int[mask != 0].sum())
    got = oracle_mod.sum_add_many_conditional(col, mask)[0]
    assert got.dtype == np.float64 and float(got) == float(exact) and int(got) == exact
    # ... in another order as well
    assert float(np.sum(col[mask != 0][::-1].astype(np.float64))) == float(exact)


@pytest.mark.parametrize("dtype", SC.ALL_DTYPES, ids=SC.name)
def test_filter_sum_reference_equals_python_arithmetic(oracle_mod, dtype):
    """cmp_const -> count_bytes_in_filter / sum_add_many_conditional (the GPU module's reference) against Python integers"""
    O = oracle_mod
    n = 1500
    rows = SC.all_edge_rows([(256, 2, 4)], lambda R, G, v: SC.size_list(R, G, v, seed=1))
    b = SC.plant(SC.uniform_column(dtype, n, 11), rows)
    a = SC.plant(SC.uniform_column(dtype, n, 12), rows, shift=2)
    t = SC.threshold(dtype)
    assert {int(x) for x in SC.planted_values(dtype)} <= {int(x) for x in b.tolist()}                # min, max, thr - 1, thr, thr + 1 are present
    kind = np.dtype(dtype).kind
    scalars = [(float(t) if kind == "f" else t, None), (t + 0.5 if abs(t) < 2 ** 52 else -0.5, F64), (max(t, 0) if t < 2 ** 63 else 5, I64 if kind != "i" else U64)]
    cond = SC.mask_column(n, 13)
    assert set(np.unique(cond).tolist()) > {0, 1} and int(cond.max()) == 255
    for op in range(6):
        for s, tag in scalars:
            mask = O.cmp_const(b, op, s, tag)
            assert mask.tolist() == [int(k) for k in SC.py_pass(b, op, s)], (SC.name(dtype), op, s)
            for val in (b, a):
                got = O.sum_add_many_conditional(val, mask)[0]
                want, cnt = SC.py_filter_sum(b, op, s, val)
                assert O.count_bytes_in_filter(mask) == cnt and got.dtype == O.sum_result_dtype(O.TAG_OF[np.dtype(dtype)])
                assert (float(got) if kind == "f" else int(got)) == want, (SC.name(dtype), op, s)
    got = O.sum_add_many_conditional(a, cond)[0]
    want, cnt = SC.py_filter_sum(a, None, None, a, mask=cond)
    assert (float(got) if kind == "f" else int(got)) == want and O.count_bytes_in_filter(cond) == cnt == int((cond != 0).sum())
    st = np.array([123], dtype=got.dtype)
    O.sum_add_many(a, 3, 700, st)
    O.sum_add_many(a, 700, n, st)
    tot = sum(a[3:].tolist()) + 123
    assert (float(st[0]) if kind == "f" else int(st[0])) == (tot if kind == "f" else SC.wrap64(tot, kind == "i"))


def test_uniform_integer_columns_use_the_whole_range_and_overflow_the_sum():
    for d in SC.INT_DTYPES:
        c = SC.uniform_column(d, 200_000, 21)
        lo, hi = SC.limits(d)
        assert c.dtype == np.dtype(d) and int(c.min()) < lo + (hi - lo) // 1000 + 1 and int(c.max()) > hi - (hi - lo) // 1000 - 1
        assert 0.45 < float((c.astype(np.float64) < SC.threshold(d)).mean()) < 0.55
    big = SC.uniform_column(np.uint64, 1000, 22).tolist()
    assert sum(big) >= 2 ** 64                                                           # the modulo-2^64 sum is exercised
    r = SC.rough_float_column(np.float64, 100_000, 23)
    assert (r < 0).any() and (r > 0).any() and np.abs(r).max() / np.abs(r[r != 0]).min() > 1e9


def test_expression_reference_equals_python_arithmetic(oracle_mod):
    """expr_filter_sum_pipeline against Python integers for every value operator over every ordered pair of operand types, with
    constants inside, at and outside the column's range; result signedness against cho_arith_sum_type"""
    O = oracle_mod
    n = 700
    tag_of = {np.dtype(np.int64): I64, np.dtype(np.uint64): U64, np.dtype(np.float64): F64}
    for ia, ta in enumerate(SC.EXPR_DTYPES):
        for ib, tb in enumerate(SC.EXPR_DTYPES):
            cols = [SC.uniform_column(ta, n, 30 + ia), SC.uniform_column(tb, n, 40 + ib), SC.uniform_column(np.uint8, n, 50)]
            preds = [(2, GE, 32), (1, NE, SC.threshold(tb))]
            for vop in (SC.VAL_COL, SC.VAL_MUL, SC.VAL_PLUS, SC.VAL_MINUS):
                for va, vb in ((0, 1), (1, 0), (0, 0)):
                    s, c = O.expr_filter_sum_pipeline(cols, preds, vop, va, vb)
                    ps, pc, signed = SC.py_expr_filter_sum(cols, preds, vop, va, vb)
                    assert (int(s), c) == (ps, pc) and (s.dtype == np.int64) == signed, (SC.name(ta), SC.name(tb), vop, va, vb)
                    if vop != SC.VAL_COL:
                        rt = O.lib().cho_arith_sum_type(vop, O.TAG_OF[cols[va].dtype], O.TAG_OF[cols[vb].dtype])
                        assert np.dtype(O.NP_OF[rt]) == s.dtype
    for d in SC.EXPR_DTYPES:
        col = SC.plant(SC.uniform_column(d, n, 60), range(0, n, 7))
        lo, hi = SC.limits(d)
        consts = SC.fold_constants(d)
        assert any(v > hi for v, _ in consts) and any(v < lo for v, _ in consts) and any(isinstance(v, float) and v != int(v) for v, _ in consts if abs(v) < 1e20)
        assert any(np.dtype(t) == np.dtype(np.uint64) and v >= 2 ** 63 for v, t in consts) and any(np.dtype(t) == np.dtype(np.int64) and v < 0 for v, t in consts)
        for scalar, sdt in consts:
            tag = None if np.dtype(sdt) == np.dtype(d) else tag_of[np.dtype(sdt)]
            for op in range(6):
                s, c = O.expr_filter_sum_pipeline([col], [(0, op, scalar, tag)], SC.VAL_COL, 0)
                ps, pc, _ = SC.py_expr_filter_sum([col], [(0, op, scalar)], SC.VAL_COL, 0)
                assert (int(s), c) == (ps, pc), (SC.name(d), op, scalar, SC.name(sdt))
    s, c = O.expr_filter_sum_pipeline([SC.uniform_column(np.int32, n, 61)], [], SC.VAL_COL, 0)       # no predicate at all
    assert c == n and int(s) == sum(SC.uniform_column(np.int32, n, 61).tolist())


def test_float_specials_reference_follows_ieee(oracle_mod):
    O = oracle_mod
    p = np.array([np.nan, 1.0, -0.0, np.inf, -np.inf, 0.0], dtype=np.float64)
    want = {EQ: [0, 0, 1, 0, 0, 1], NE: [1, 1, 0, 1, 1, 0], LT: [0, 0, 0, 0, 1, 0], GT: [0, 1, 0, 1, 0, 0], LE: [0, 0, 1, 0, 1, 1], GE: [0, 1, 1, 1, 0, 1]}
    for op, w in want.items():
        assert O.cmp_const(p, op, 0.0).tolist() == w
        assert O.cmp_const(p, op, float("nan")).tolist() == ([1] * 6 if op == NE else [0] * 6)
        assert O.cmp_const(p.astype(np.float32), op, 0.0, F64).tolist() == w
    ones = np.ones(6, dtype=np.uint8)
    assert np.isnan(O.sum_add_many_conditional(p, ones)[0]) and np.isnan(O.sum_add_many_conditional(p[3:], ones[3:])[0])
    assert O.sum_add_many_conditional(p[1:4], ones[1:4])[0] == np.inf
    z = O.sum_add_many_conditional(np.full(5, -0.0), np.ones(5, dtype=np.uint8))[0]
    assert z == 0.0 and math.copysign(1.0, float(z)) == math.copysign(1.0, float(np.sum(np.full(5, -0.0)) + 0.0))
    f = np.array([0.1, 0.25], dtype=np.float32)
    assert O.cmp_const(f, EQ, 0.1, F64).tolist() == [0, 0] and O.cmp_const(f, GT, 0.1, F64).tolist() == [1, 1] and O.cmp_const(f, EQ, float(np.float32(0.1)), F64).tolist() == [1, 0]
