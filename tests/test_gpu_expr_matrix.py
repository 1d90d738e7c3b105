"""The run-time expression compiler (csrc/expr_jit.hip) on the device, systematically: every accepted (function, operand types)
combination over adversarial values (tests/expr_cases.py: 1506 computed as written + 174 commutative mirror images, in 106 kernels),
the calendar over every day number, and every launch shape of its four kernel families -- the vector widths of k_run, its LDS
transpose of one-byte outputs, ragged tails, unaligned views (one row per lane), the loops that run when there are more chunks than
workgroups, the fused filter + sum, filter + min / max and WHERE + projection.  Integers must be equal, floats bit for bit."""
import numpy as np
import pytest

import expr_cases as XC
from oracle import expr_dag as OE

pytestmark = pytest.mark.gpu
MATRIX_ROWS = 40_001  # two full chunks at 16 rows per lane (16384 rows each) and a ragged tail


def _ch():
    import clickhouse_amd as ch
    return ch


def _num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _compile(nodes):
    d = _ch().ActionsDAG()
    d.nodes = list(nodes)
    return d.compile()


def _check_outputs(ex, ctx, cols, nodes, out_nodes, want, label, kernel=None):
    outs = ex.execute(ctx, cols, out_nodes)
    for o, (k, col) in enumerate(zip(out_nodes, outs)):
        got = col.numpy()
        if not XC.same(got, want[k]):
            names = XC.mismatches(kernel, o, got, want[k]) if kernel is not None else []
            bad = np.flatnonzero(~((got == want[k]) | ((got != got) & (want[k] != want[k]))))[:4] if got.shape == want[k].shape else []
            pytest.fail(f"{label}: output {o} (node {k} {nodes[k][:2]}) differs: {names[:6]} rows {list(bad)} got {got[bad]} want {want[k][bad]}")


# ----------------------------------------------------------------------------------------------------------------------
# the calendar
# ----------------------------------------------------------------------------------------------------------------------
def test_calendar_every_day_number_against_datetime():
    ctx = _ch().Context()
    ref = XC.calendar_reference()
    nodes = XC.calendar_nodes()
    ex = _compile(nodes)
    days = np.arange(65536, dtype=np.uint16)
    host = np.concatenate([days[-1:], days])  # one row in front: the view cut one row in is every day number again
    col = ctx.upload(host)
    for view, label in ((ctx.upload(days), "aligned"), (col.cut(1, 65536), "unaligned")):
        outs = ex.execute(ctx, [view], list(range(1, 9)))
        for f, o in zip(XC.CALENDAR, outs):
            got = o.numpy()
            assert got.dtype == np.dtype(XC.NP_OF[OE.result_type(XC.FN[f], XC.U16)])
            bad = np.flatnonzero(got != np.array(ref[f], dtype=got.dtype))
            assert bad.size == 0, (f, label, bad[:4], got[bad[:4]], [ref[f][i] for i in bad[:4]])


# ----------------------------------------------------------------------------------------------------------------------
# the fused filter + sum
# ----------------------------------------------------------------------------------------------------------------------
def _fsum_dag(t, passing="half"):
    """c0: the values, c1: a UInt32 row selector; -> (nodes, filter node, value node)"""
    d = XC._Dag([t, XC.U32])
    v, s = d.inp(0), d.inp(1)
    if passing == "half":
        f = d.fn(XC.FN["less"], s, d.const(2**31, XC.U32))
    elif passing == "none":
        f = d.fn(XC.FN["less"], s, d.const(0, XC.U32))
    else:
        f = d.fn(XC.FN["greaterOrEquals"], s, d.const(0, XC.U32))
    return d.nodes, f, v


def _fsum_values(rng, t, n):
    if XC.is_float(t):  # k / 8 with |k| < 2^20 over at most 2^20 rows: every partial sum is exact in Float64, in any order
        assert n <= 2**20
        k = rng.integers(-(2**20) + 1, 2**20, size=n)
        return (k / 8.0).astype(XC.NP_OF[t]), k
    x = XC.random_column(rng, t, n)
    return x, x


def _fsum_expected(t, k, keep):
    """exact, on Python integers: Float sums as (sum of k) / 8, integer sums modulo 2^64 in the sum's type"""
    tot = sum(k[keep].tolist())
    if XC.is_float(t):
        return np.float64(tot / 8.0)
    return np.uint64(tot % 2**64) if t not in XC.SIGNED_INT else np.int64(XC.wrap(tot, XC.I64))


@pytest.mark.parametrize("t", XC.TAGS, ids=lambda t: XC.NAME[t])
def test_filter_sum_every_value_type(t):
    from clickhouse_amd.columns import sum_result_dtype
    ctx = _ch().Context()
    rng = np.random.Generator(np.random.PCG64(100 + t))
    n = MATRIX_ROWS
    x, k = _fsum_values(rng, t, n + 1)
    sel = rng.integers(0, 2**32, size=n + 1, dtype=np.uint32)
    if not XC.is_float(t) and XC.BITS[t] < 64:
        assert (x < 0).any() or t not in XC.SIGNED_INT  # negative narrow values: sign extension into the 64-bit accumulator
    nodes, f, v = _fsum_dag(t)
    ex = _compile(nodes)
    cx, cs = ctx.upload(x), ctx.upload(sel)
    for lo, rows, label in ((0, n, "aligned"), (1, n, "unaligned"), (0, 1, "one row"), (5, 1, "one row, unaligned")):
        keep = np.zeros(n + 1, dtype=bool)
        keep[lo:lo + rows] = sel[lo:lo + rows] < 2**31
        s, c = ex.filter_sum(ctx, [cx.cut(lo, rows), cs.cut(lo, rows)], f, v)
        want = _fsum_expected(t, k, keep)
        assert s.dtype == np.dtype(sum_result_dtype(t)) == want.dtype, label
        print(f"{XC.NAME[t]} {label}: sum {s!r} want {want!r} count {c} want {int(keep.sum())}")
        assert c == int(keep.sum()), label
        assert s.tobytes() == want.tobytes(), (label, s, want)  # bit-exact, Float sums included
    assert 0.4 * n < int((sel[:n] < 2**31).sum()) < 0.6 * n


def test_filter_sum_edges_and_more_chunks_than_workgroups():
    ctx = _ch().Context()
    rng = np.random.Generator(np.random.PCG64(7))
    t = XC.I32
    v_rows = XC.vec_rows([t, XC.U32])
    n_big = _num_cus() * XC.chunk_rows(v_rows) + 2 * XC.chunk_rows(v_rows) + 77
    x = XC.random_column(rng, t, n_big)
    sel = rng.integers(0, 2**32, size=n_big, dtype=np.uint32)
    cx, cs = ctx.upload(x), ctx.upload(sel)
    n = MATRIX_ROWS
    cols = [cx.cut(0, n), cs.cut(0, n)]
    every = np.ones(n, dtype=bool)
    for passing, keep in (("none", ~every), ("all", every)):
        nodes, f, v = _fsum_dag(t, passing)
        ex = _compile(nodes)
        s, c = ex.filter_sum(ctx, cols, f, v)
        assert (int(s), c) == (int(_fsum_expected(t, x[:n], keep)), int(keep.sum())) and s.dtype == np.int64, passing
    nodes, f, v = _fsum_dag(t)
    ex = _compile(nodes)
    s, c = ex.filter_sum(ctx, cols, -1, v)  # no filter
    assert (int(s), c) == (int(_fsum_expected(t, x[:n], every)), n)
    s, c = ex.filter_sum(ctx, cols, f, -1)  # count only
    assert (int(s), c) == (0, int((sel[:n] < 2**31).sum())) and s.dtype == np.uint64
    s, c = ex.filter_sum(ctx, cols, -1, -1)
    assert (int(s), c) == (0, n)
    # one workgroup per compute unit and more chunks than workgroups: the `ch += gridDim.x` loop of the sum form runs
    ctx1 = _ch().Context()
    ctx1.set_option("tune_jit_wg_sum", 1)
    assert n_big // XC.chunk_rows(v_rows) > _num_cus()
    c1x, c1s = ctx1.upload(x), ctx1.upload(sel)
    keep = sel < 2**31
    s, c = ex.filter_sum(ctx1, [c1x, c1s], f, v)
    assert (int(s), c) == (int(_fsum_expected(t, x, keep)), int(keep.sum()))


# ----------------------------------------------------------------------------------------------------------------------
# the fused filter + min / max
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", XC.INTS, ids=lambda t: XC.NAME[t])
def test_filter_minmax_every_integer_type(t):
    ctx = _ch().Context()
    rng = np.random.Generator(np.random.PCG64(200 + t))
    dt = XC.NP_OF[t]
    info = np.iinfo(dt)
    n_big = _num_cus() * 8 * 256 * 4 + 777  # past one turn of the `i0 += stride * 4` loop
    x = rng.integers(int(info.min) + 1, int(info.max) - 1, size=n_big, dtype=dt, endpoint=True)
    n = MATRIX_ROWS
    # the extremes in different lanes, waves and workgroups, and in different quarters of a thread's four rows
    x[[5, 30_000]] = info.min
    x[[10_300, 39_999]] = info.max
    x[[n_big - 3, n_big // 2 + 1]] = info.min, info.max
    d = XC._Dag([t])
    v = d.inp(0)
    f_mid = d.fn(XC.FN["and"], d.fn(XC.FN["notEquals"], v, d.const(int(info.min), t)), d.fn(XC.FN["notEquals"], v, d.const(int(info.max), t)))
    f_none = d.fn(XC.FN["less"], v, d.const(int(info.min), t))
    ex = _compile(d.nodes)
    col = ctx.upload(x)
    for rows in (n, n_big):
        view, h = col.cut(0, rows), x[:rows]
        lo, hi, c = ex.filter_minmax(ctx, [view], -1, v)
        assert lo.dtype == np.dtype(dt) and (int(lo), int(hi), c) == (int(info.min), int(info.max), rows), rows
        mid = h[(h != info.min) & (h != info.max)]
        lo, hi, c = ex.filter_minmax(ctx, [view], f_mid, v)  # the filter excludes exactly the extremes
        assert (int(lo), int(hi), c) == (int(mid.min()), int(mid.max()), mid.shape[0]) and c < rows, rows
        assert ex.filter_minmax(ctx, [view], f_none, v) == (0, 0, 0)
    for row in (5, 6, 10_300):  # one row, at an unaligned address too
        lo, hi, c = ex.filter_minmax(ctx, [col.cut(row, 1)], -1, v)
        assert (int(lo), int(hi), c) == (int(x[row]), int(x[row]), 1)


def test_filter_minmax_of_a_float_node_is_not_implemented():
    ch = _ch()
    ctx = ch.Context()
    d = XC._Dag([XC.F64])
    v = d.fn(XC.FN["negate"], d.inp(0))
    ex = _compile(d.nodes)
    with pytest.raises(ch.ChgpuError) as ei:
        ex.filter_minmax(ctx, [ctx.upload(np.arange(4, dtype=np.float64))], -1, v)
    assert ei.value.code == ch._capi.ERR_NOT_IMPLEMENTED


# ----------------------------------------------------------------------------------------------------------------------
# the kernel shapes of execute
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", XC.shape_cases(), ids=lambda c: c.name)
def test_execute_kernel_shapes(case):
    ctx = _ch().Context()
    rng = np.random.Generator(np.random.PCG64(300 + case.v))
    r = XC.chunk_rows(case.v)
    cus = _num_cus()
    n_big = cus * r + r + 64 * case.v + 5
    host = [XC.random_column(rng, t, n_big + 1) for t in case.in_types]
    want, types = OE.evaluate(case.nodes, host)  # once: every function is row-wise, so a window of the result is the result of the window
    ex = _compile(case.nodes)
    assert [ex.node_type(k) for k in case.out_nodes] == [types[k] for k in case.out_nodes]
    up = [ctx.upload(h) for h in host]
    for lo in (0, 1):  # 0: aligned, V rows per lane; 1: a view cut one row in, one row per lane
        sizes = XC.shape_sizes(case.v) if lo == 0 else sorted(set(XC.shape_sizes(case.v) + XC.shape_sizes(1)))
        for n in sizes:
            _check_outputs(ex, ctx, [c.cut(lo, n) for c in up], case.nodes, case.out_nodes, [w[lo:lo + n] for w in want],
                           f"{case.name} rows {n} from {lo}")
    outs = ex.execute(ctx, [c.cut(0, 0) for c in up], case.out_nodes)  # no rows: empty columns of the right types
    assert [(o.size(), OE.TAG_OF[o.dtype]) for o in outs] == [(0, types[k]) for k in case.out_nodes]
    # one workgroup per compute unit and more chunks than workgroups: the `ch += gridDim.x` loop of the map form runs
    ctx1 = _ch().Context()
    ctx1.set_option("tune_jit_wg_map", 1)
    assert n_big // r > cus
    up1 = [ctx1.upload(h) for h in host]
    for lo in ((0, 1) if case.v == 2 else (0,)):  # one row per lane: 1024 rows per chunk, so n_big is past its loop as well
        _check_outputs(ex, ctx1, [c.cut(lo, n_big) for c in up1], case.nodes, case.out_nodes, [w[lo:lo + n_big] for w in want],
                       f"{case.name} rows {n_big} from {lo}, one workgroup per CU")


# ----------------------------------------------------------------------------------------------------------------------
# WHERE + projection
# ----------------------------------------------------------------------------------------------------------------------
def _projection_dag():
    """c0 UInt32, c1 Int16, c2 the UInt8 filter column -> 7 outputs of 1, 2, 4 and 8 bytes, a Float64, an INPUT and a CONST"""
    d = XC._Dag([XC.U32, XC.I16, XC.U8])
    a, b, f = d.inp(0), d.inp(1), d.inp(2)
    outs = [d.fn(XC.FN_CAST + XC.I8, b), b, d.fn(XC.FN["bitXor"], a, d.const(0x9E3779B9, XC.U32)), d.fn(XC.FN["multiply"], a, b),
            d.fn(XC.FN["divide"], a, b), d.const(40_000, XC.U16), d.fn(XC.FN["plus"], b, b)]
    assert sorted(XC.BITS[d.types[k]] for k in outs) == [8, 16, 16, 32, 32, 64, 64]
    return d.nodes, f, outs


def _filters(n):
    alt = (np.arange(n) % 2).astype(np.uint8) * 255
    two = np.zeros(n, dtype=np.uint8)
    two[np.array([i for i in (1023, 1024) if i < n], dtype=np.intp)] = 1
    last = np.zeros(n, dtype=np.uint8)
    last[n - 1] = 7
    return {"none": np.zeros(n, dtype=np.uint8), "all": np.full(n, 3, dtype=np.uint8), "alternating": alt, "rows 1023 and 1024": two, "last": last}


def test_filter_execute_surviving_rows_in_order():
    ctx = _ch().Context()
    rng = np.random.Generator(np.random.PCG64(41))
    nodes, f, outs = _projection_dag()
    ex = _compile(nodes)
    n_max = 3 * 1024 + 1
    a, b = XC.random_column(rng, XC.U32, n_max + 1), XC.random_column(rng, XC.I16, n_max + 1)
    ca, cb = ctx.upload(a), ctx.upload(b)
    for lo in (0, 1):
        for n in (1, 1023, 1024, 1025, n_max):
            for name, filt in _filters(n).items():
                host = [a[lo:lo + n], b[lo:lo + n], filt]
                want, _ = OE.evaluate(nodes, host)
                cf = ctx.upload(np.concatenate([filt[:1], filt])).cut(1, n) if lo else ctx.upload(filt)
                got, rows = ex.filter_execute(ctx, [ca.cut(lo, n), cb.cut(lo, n), cf], f, outs)
                keep = filt != 0
                assert rows == int(keep.sum()), (lo, n, name)
                for k, o in zip(outs, got):
                    assert XC.same(o.numpy(), want[k][keep]), (lo, n, name, nodes[k][:2])


def test_filter_execute_a_wave_takes_a_second_chunk():
    ctx = _ch().Context()
    rng = np.random.Generator(np.random.PCG64(42))
    n = _num_cus() * 8 * 4 * 1024 + 1025  # 8 workgroups per compute unit, 4 waves each, 1024 rows per wave and turn
    x = rng.integers(0, 256, size=n, dtype=np.uint8)
    x[rng.integers(0, n, size=n // 2)] = 0
    d = XC._Dag([XC.U8])
    neg = d.fn(XC.FN["negate"], d.inp(0))
    assert len(d.nodes) == 2
    ex = _compile(d.nodes)
    got, rows = ex.filter_execute(ctx, [ctx.upload(x)], d.inp(0), [neg])
    want = -(x[x != 0].astype(np.int16))
    assert rows == want.shape[0] and 0.3 * n < rows < 0.7 * n
    assert XC.same(got[0].numpy(), want)


# ----------------------------------------------------------------------------------------------------------------------
# the function matrix
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", XC.pairs(), ids=lambda p: XC.pair_id(*p))
def test_function_matrix(pair):
    a, b = pair
    ctx = _ch().Context()
    n = MATRIX_ROWS
    host = list(XC.cross_columns(a, b, n + 1))
    assert n >= 3 * len(XC.VALUES[a]) * len(XC.VALUES[b])  # every value pair under every condition
    up = [ctx.upload(h) for h in host]
    for ki, k in enumerate(XC.plan()[0][pair]):
        with np.errstate(all="ignore"):
            want, types = OE.evaluate(k.nodes, host)
        assert types == k.types
        ex = _compile(k.nodes)
        assert [ex.node_type(j) for j in range(len(k.nodes))] == k.types
        used = {nd[1] for nd in k.nodes if nd[0] == XC.EX_INPUT}
        for lo in ((0, 1) if ki == 0 else (0,)):  # the first kernel again on views cut one row in: one row per lane, the same values
            cols = [c.cut(lo, n) if j in used else None for j, c in enumerate(up)]
            _check_outputs(ex, ctx, cols, k.nodes, k.out_nodes, [w[lo:lo + n] for w in want], f"{XC.pair_id(a, b)} kernel {ki} from row {lo}", k)
