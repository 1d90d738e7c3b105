"""The -If combinator and Nullable arguments of the GROUP BY aggregates on the device (chgpu_agg_set_conditions,
chgpu_agg_execute_on_block_conditional, chgpu_agg_finalize_nullable) against the row-order restatement in tests/agg_conditions_ref.py.
Integer results, counts, min / max / any / argMin / argMax and null maps are compared bit for bit, Float64 sums bit for bit against
math.fsum (the values are multiples of a power of two well inside the fixed-point window, so both are exact), avg with rtol 1e-6 and NaN
matching NaN.  Every keyed input holds the zero key, a group whose rows fail every condition and are all NULL, and a group whose rows
all pass: _assert_special_groups checks that before the device is touched."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import agg_conditions_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
DEAD, LIVE = 77_001, 77_002   # the group no function ever sees a row of / the group whose rows all pass


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _special(keys, conds, modes):
    """force the three special groups into (a copy of) the condition columns: rows of DEAD fail / are NULL, rows of LIVE pass"""
    out = []
    for c, m in zip(conds, modes):
        if c is None:
            out.append(None)
            continue
        c = c.copy()
        c[keys == DEAD] = 0 if m == "if" else 1
        c[keys == LIVE] = 3 if m == "if" else 0
        out.append(c)
    return out


def _assert_special_groups(blocks, modes, dead=DEAD, live=LIVE):
    """blocks: [(keys, conds, where or None)]"""
    keys = np.concatenate([k if w is None else k[w != 0] for k, _, w in blocks])
    assert (keys == 0).any() and (keys == dead).any() and (keys == live).any()
    for j, m in enumerate(modes):
        if m is None:
            continue
        c = np.concatenate([cs[j] if w is None else cs[j][w != 0] for _, cs, w in blocks])
        reach = (c != 0) if m == "if" else (c == 0)
        assert not reach[keys == dead].any() and reach[keys == live].all(), j


def _compare(got, ref):
    """got = Aggregator.convert_to_block(null_maps=True); every group and every function is compared"""
    keys, res, maps = got
    klist = [None] if keys is None else keys.tolist()
    assert sorted(klist, key=lambda k: -1 if k is None else k) == sorted(ref.groups, key=lambda k: -1 if k is None else k)
    want, want_maps = ref.columns(klist)
    for j, (kind, _, mode) in enumerate(ref.aggs):
        assert res[j].dtype == want[j].dtype, j
        if kind == R.AVG:
            np.testing.assert_allclose(res[j], want[j], rtol=1e-6, atol=0, equal_nan=True, err_msg=f"aggregate {j}")
        else:
            assert res[j].tobytes() == want[j].tobytes(), (j, res[j], want[j])
        if want_maps[j] is None:
            assert maps[j] is None, j
        else:
            assert maps[j].dtype == np.uint8 and maps[j].tobytes() == want_maps[j].tobytes(), (j, maps[j], want_maps[j])


def _values(rng, dtype, n):
    """argument values; floats are multiples of 2^-8 below 2^20: every partial sum is exact in Float64 and in the fixed-point window"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.integers(-(1 << 27), 1 << 27, size=n) / 256.0).astype(dt) if dt == np.float64 else (rng.integers(-(1 << 15), 1 << 15, size=n) / 16.0).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)


# ---- 1. lanes and bytes --------------------------------------------------------------------------------------------------------------
FIVE = [R.COUNT, R.SUM, R.AVG, R.MIN, R.MAX]
THREE = [R.ANY, R.ARG_MIN, R.ARG_MAX]


@pytest.mark.parametrize("mode", ["if", "null"])
@pytest.mark.parametrize("dtype", ["int64", "uint32", "int8", "float64", "float32"])
@pytest.mark.parametrize("groups", [1, 1000])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_lanes_and_condition_bytes(ch, n, groups, dtype, mode):
    rng = _rng(n * 31 + groups + len(dtype) + len(mode))
    ctx = ch.Context(0)
    # a preamble block holds the three special groups; the n-row block follows, once whole and once as the view [1, n - 1)
    pk = np.array([0, DEAD, DEAD, LIVE, LIVE], dtype=np.uint64)
    bk = rng.integers(1, groups + 1, size=n).astype(np.uint64) if groups > 1 else np.full(n, 5, dtype=np.uint64)
    i = np.arange(n)
    flip = ((i < 63) | (i == 64) | ((i > 65) & (rng.random(n) < 0.5))).astype(np.uint8)   # 1 ... 1, 0 at 63, 1 at 64, 0 at 65
    flip = flip if mode == "if" else (1 - flip).astype(np.uint8)
    byte = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=n)
    for kinds in (FIVE, THREE):
        aggs = [(k, (dtype, "int64") if k in (R.ARG_MIN, R.ARG_MAX) else None if k == R.COUNT else dtype, mode) for k in kinds]
        modes = [mode] * len(aggs)
        blocks = []
        for keys in (pk, bk):
            m = len(keys)
            x, v = _values(rng, dtype, m), rng.integers(-3, 4, size=m)   # val: few distinct values, many ties
            conds = [(flip if j % 2 == 0 else byte) if keys is bk else np.ones(m, dtype=np.uint8) for j in range(len(aggs))]
            conds = _special(keys, conds, modes)
            args = [(x, v) if k in (R.ARG_MIN, R.ARG_MAX) else None if k == R.COUNT else x for k in kinds]
            blocks.append((keys, conds, None, args))
        _assert_special_groups([b[:3] for b in blocks], modes)
        view = (1, n - 1) if n >= 3 else (0, n)   # (a one-row block has no inner view)
        for rb, re in ((0, n), view):
            ag = ch.Aggregator(np.uint64, aggs, ctx=ctx)
            ref = R.Ref(aggs)
            for bi, (keys, conds, _, args) in enumerate(blocks):
                b, e = (rb, re) if bi == 1 else (0, len(keys))
                ag.execute_on_block(keys, args, row_begin=b, row_end=e, conds=conds)
                ref.add_block(keys, args, conds=conds, row_begin=b, row_end=e)
            _compare(ag.convert_to_block(null_maps=True), ref)


# ---- 2. empty states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["if", "null"])
def test_extreme_values_against_empty_states(ch, mode):
    ctx = ch.Context(0)
    keys = np.array([0, 0, 1, 1, 2, 2, DEAD, DEAD, LIVE], dtype=np.uint32)
    vmin = np.array([I64_MAX, 5, I64_MAX, I64_MIN, 7, 8, I64_MIN, 1, I64_MAX], dtype=np.int64)
    vmax = np.array([I64_MIN, 5, I64_MIN, I64_MAX, 7, 8, I64_MAX, 1, I64_MIN], dtype=np.int64)
    reach = np.array([1, 0, 1, 0, 0, 0, 0, 0, 1], dtype=np.uint8)   # key 0 / 1: only the extreme row; key 2 and DEAD: no row
    c = reach if mode == "if" else (1 - reach).astype(np.uint8)
    aggs = [(R.MIN, np.int64, mode), (R.MAX, np.int64, mode), (R.AVG, np.int64, mode), (R.SUM, np.int64, mode), (R.COUNT, None, mode)]
    conds = [c] * 5
    _assert_special_groups([(keys, conds, None)], [mode] * 5)
    args = [vmin, vmax, vmin, vmin, None]
    ag = ch.Aggregator(np.uint32, aggs, ctx=ctx)
    ag.execute_on_block(keys, args, conds=conds)
    ref = R.Ref(aggs)
    ref.add_block(keys, args, conds=conds)
    got = ag.convert_to_block(null_maps=True)
    _compare(got, ref)
    k, res, maps = got
    at = {int(x): i for i, x in enumerate(k.tolist())}
    assert res[0][at[0]] == I64_MAX and res[1][at[0]] == I64_MIN       # the type's extremum is a value ...
    assert res[0][at[2]] == 0 and res[1][at[2]] == 0                   # ... and no row at all is the default
    if mode == "if":
        assert math.isnan(res[2][at[2]]) and maps == [None] * 5
    else:
        assert res[2][at[2]] == 0.0 and maps[2][at[2]] == 1 and maps[0][at[2]] == 1 and maps[0][at[0]] == 0 and maps[4] is None


@pytest.mark.parametrize("mode", ["if", "null"])
def test_a_masked_out_row_holds_the_better_value(ch, mode):
    ctx = ch.Context(0)
    n = 3000
    rng = _rng(5)
    keys = np.concatenate([np.array([0, DEAD, LIVE], dtype=np.uint64), rng.integers(0, 40, size=n).astype(np.uint64)])
    arg = np.arange(len(keys), dtype=np.int64) + 100
    val = rng.integers(0, 6, size=len(keys)).astype(np.int32)
    reach = (rng.random(len(keys)) < 0.4).astype(np.uint8)
    # the earliest row of every group and every row that holds the group's best val are masked out
    first = np.unique(keys, return_index=True)[1]
    reach[first] = 0
    reach[(val == 5) | (val == 0)] = 0
    c = reach if mode == "if" else (1 - reach).astype(np.uint8)
    aggs = [(R.ANY, np.int64, mode), (R.ARG_MAX, (np.int64, np.int32), mode), (R.ARG_MIN, (np.int64, np.int32), mode)]
    conds = _special(keys, [c] * 3, [mode] * 3)
    _assert_special_groups([(keys, conds, None)], [mode] * 3)
    args = [arg, (arg, val), (arg, val)]
    ag = ch.Aggregator(np.uint64, aggs, ctx=ctx)
    ref = R.Ref(aggs)
    for b, e in ((0, 1500), (1500, len(keys))):
        ag.execute_on_block(keys, args, row_begin=b, row_end=e, conds=conds)
        ref.add_block(keys, args, conds=conds, row_begin=b, row_end=e)
    _compare(ag.convert_to_block(null_maps=True), ref)


# ---- 3. several functions, shared and distinct conditions, every small-cardinality plan ----------------------------------------------
def _plan_lines(err):
    return [ln for ln in err.splitlines() if ln.startswith("chgpu: ") and "GROUP BY" in ln and "finish rounds" not in ln]


@pytest.fixture(scope="module")
def dashboard():
    """sum(a), sumIf(a, c1), sumIf(a, c2), sumIf(b, c1), countIf(c2), avgIf(b, c2), count(): the same column under two conditions, more
    argument words than one ranged pass holds; the reference is computed once"""
    rng = _rng(33)
    n, G = 200_000, 1000
    keys = rng.integers(0, G - 2, size=n).astype(np.uint32)
    keys[:40] = DEAD
    keys[40:80] = LIVE
    keys = rng.permutation(keys)
    a = rng.integers(-(1 << 40), 1 << 40, size=n)
    b = rng.integers(0, 1 << 32, size=n).astype(np.uint32)
    c1 = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=n)
    c2 = (rng.random(n) < 0.1).astype(np.uint8)
    where = (rng.random(n) < 0.6).astype(np.uint8)
    where[(keys == DEAD) | (keys == LIVE) | (keys == 0)] = 1
    aggs = [(R.SUM, np.int64), (R.SUM, np.int64, "if"), (R.SUM, np.int64, "if"), (R.SUM, np.uint32, "if"), (R.COUNT, None, "if"), (R.AVG, np.uint32, "if"),
            (R.COUNT, None)]
    modes = [None, "if", "if", "if", "if", "if", None]
    c1, c2 = _special(keys, [c1, c2], ["if", "if"])
    conds = [None, c1, c2, c1, c2, c2, None]   # a shared column is the same object (and one device column)
    args = [a, a, a, b, None, b, None]
    out = {"n": n, "keys": keys, "args": args, "conds": conds, "where": where, "aggs": aggs, "modes": modes}
    for name, w in (("want_all", None), ("want_where", where)):
        _assert_special_groups([(keys, conds, w)], modes)
        out[name] = R.additive_reference(keys, args, conds, aggs, where=w)
    return out


def _check_additive(got, want):
    keys, res, maps = got
    gk, vals, nulls = want
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(keys[order], gk)
    for j in range(len(vals)):
        if vals[j].dtype == np.float64:
            np.testing.assert_allclose(res[j][order], vals[j], rtol=1e-6, atol=0, equal_nan=True, err_msg=f"aggregate {j}")
        else:
            assert res[j].dtype == vals[j].dtype and np.array_equal(res[j][order], vals[j]), j
        assert (maps[j] is None) == (nulls[j] is None) and (nulls[j] is None or np.array_equal(maps[j][order], nulls[j])), j


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("plan,opts,hint,frag", [("ranged", {}, 1000, "ranged GROUP BY"), ("rows_lds", {"tune_agg_no_ranged": 1}, 1000, "kernel=rows_lds"),
                                                 ("direct", {}, 1 << 17, "kernel=rows_direct")])
def test_shared_and_distinct_conditions_on_every_small_plan(ch, capfd, dashboard, plan, opts, hint, frag, filtered):
    d = dashboard
    ctx = ch.Context(0)
    for name, value in opts.items():
        ctx.set_option(name, value)
    ctx.set_option("debug", 1)
    ag = ch.Aggregator(np.uint32, d["aggs"], size_hint=hint, ctx=ctx)
    up = {}
    col = lambda x: None if x is None else up.setdefault(id(x), ctx.upload(x))   # a shared column is one device column
    capfd.readouterr()
    ag.execute_on_block(col(d["keys"]), [col(x) for x in d["args"]], conds=[col(c) for c in d["conds"]], filter=col(d["where"]) if filtered else None)
    err = capfd.readouterr().err
    assert any(frag in ln for ln in _plan_lines(err)), err
    _check_additive(ag.convert_to_block(null_maps=True), d["want_where" if filtered else "want_all"])


# ---- 4. large cardinality ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    rng = _rng(44)
    n, G = (4 << 20) + 77, 1 << 19
    keys = rng.integers(0, G, size=n).astype(np.uint64)
    keys[:3] = G + 1      # (DEAD and LIVE themselves lie inside [0, G) here)
    keys[3:6] = G + 2
    keys[6] = 0
    v = rng.integers(-(1 << 40), 1 << 40, size=n)
    c = (rng.random(n) < 0.5).astype(np.uint8) * rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=n)
    c[:3], c[3:6] = 0, 1
    aggs = [(R.SUM, np.int64, "if"), (R.COUNT, None, "if"), (R.AVG, np.int64, "if"), (R.SUM, np.int64)]
    args, conds = [v, None, v, v], [c, c, c, None]
    _assert_special_groups([(keys, conds, None)], ["if", "if", "if", None], dead=G + 1, live=G + 2)
    return {"keys": keys, "args": args, "conds": conds, "aggs": aggs, "want": R.additive_reference(keys, args, conds, aggs)}


@pytest.mark.parametrize("key_dtype", ["uint32", "uint64"])
def test_large_cardinality_takes_the_direct_plan(ch, capfd, large, key_dtype):
    ctx = ch.Context(0)
    ctx.set_option("debug", 1)
    ag = ch.Aggregator(key_dtype, large["aggs"], size_hint=1 << 19, ctx=ctx)
    keys = ctx.upload(large["keys"].astype(key_dtype))
    v, c = ctx.upload(large["args"][0]), ctx.upload(large["conds"][0])
    capfd.readouterr()
    ag.execute_on_block(keys, [v, None, v, v], conds=[c, c, c, None])
    err = capfd.readouterr().err
    # a conditioned aggregation of large cardinality takes the DIRECT kernel, never the partitioned plans (the same
    # aggregation without conditions takes the tile-sorted plan at this shape)
    lines = _plan_lines(err)
    assert any("kernel=rows_direct" in ln and "states=conditioned" in ln for ln in lines), err
    assert not any("partitioned GROUP BY" in ln or "tile-sorted GROUP BY" in ln for ln in lines), err
    want = (large["want"][0].astype(key_dtype), large["want"][1], large["want"][2])
    _check_additive(ag.convert_to_block(null_maps=True), want)


def test_pending_rows_rerun_under_their_conditions(ch, capfd):
    """More groups than the first table holds at max fill (the way the existing pending-row tests get there: no option shrinks the
    table): the rows left pending re-run (k_agg_rows_direct<PENDING>) under their conditions.  The 2^19 groups of the inputs above fit
    the smallest table, so this case brings its own keys."""
    rng = _rng(45)
    n, G = (5 << 20) + 13, 3 << 20   # the table starts at 4 Mi cells, max fill 2 Mi groups
    keys = rng.integers(1, G, size=n).astype(np.uint64)
    keys[:3], keys[3:6], keys[6] = G + 1, G + 2, 0
    v = rng.integers(-(1 << 40), 1 << 40, size=n)
    c = rng.choice(np.array([0, 0, 1, 255], dtype=np.uint8), size=n)
    c[:3], c[3:6] = 0, 1
    aggs = [(R.SUM, np.int64, "if"), (R.COUNT, None, "if"), (R.SUM, np.int64)]
    _assert_special_groups([(keys, [c, c, None], None)], ["if", "if", None], dead=G + 1, live=G + 2)
    ctx = ch.Context(0)
    ctx.set_option("debug", 1)
    ag = ch.Aggregator(np.uint64, aggs, size_hint=1 << 20, ctx=ctx)
    capfd.readouterr()
    ag.execute_on_block(keys, [v, None, v], conds=[c, c, None])
    err = capfd.readouterr().err
    import re
    assert "kernel=rows_direct" in err and max(int(r) for r in re.findall(r"finish rounds=(\d+)", err)) >= 1, err
    _check_additive(ag.convert_to_block(null_maps=True), R.additive_reference(keys, [v, None, v], [c, c, None], aggs))


# ---- 5. WHERE together with conditions through the materialised path -----------------------------------------------------------------
def _max_if_reference(keys, v, c, where):
    live = where != 0
    gk, inv = np.unique(keys[live], return_inverse=True)
    reach = (c != 0)[live]
    mx = np.full(len(gk), I64_MIN)
    np.maximum.at(mx, inv[reach], v[live][reach])
    cnt = np.bincount(inv[reach], minlength=len(gk))
    mx[cnt == 0] = 0
    s = np.zeros(len(gk), dtype=np.int64)
    np.add.at(s, inv[reach], v[live][reach])
    return gk, mx, s


@pytest.mark.parametrize("n,hint,kept", [(16 << 20, 1000, 0.2), ((8 << 20) + 77, 0, 0.5)])
def test_where_with_conditions_through_the_materialised_path(ch, n, hint, kept):
    """maxIf makes the aggregation DIRECT, so a WHERE mask is materialised: the condition column is filtered with the keys and
    arguments.  16 Mi rows with under 30 % kept also pass the count-then-materialise gate; (8 Mi + 77) rows without a hint take the
    sampling split, which re-enters with a shifted row_begin."""
    rng = _rng(n % 1000 + 7)
    keys = rng.integers(0, 500, size=n).astype(np.uint32)
    keys[:5], keys[5:10] = DEAD, LIVE
    v = rng.integers(-(1 << 50), 1 << 50, size=n)
    c = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=n)
    c[:5], c[5:10] = 0, 9
    where = (rng.random(n) < kept).astype(np.uint8)
    where[:10] = 1
    where[np.flatnonzero(keys == 0)[:1]] = 1
    _assert_special_groups([(keys, [c, c], where)], ["if", "if"])
    ctx = ch.Context(0)
    ag = ch.Aggregator(np.uint32, [(R.MAX, np.int64, "if"), (R.SUM, np.int64, "if")], size_hint=hint, ctx=ctx)
    cc = ctx.upload(c)
    vv = ctx.upload(v)
    ag.execute_on_block(ctx.upload(keys), [vv, vv], conds=[cc, cc], filter=ctx.upload(where))
    gk, mx, s = _max_if_reference(keys, v, c, where)
    k, res, maps = ag.convert_to_block(null_maps=True)
    order = np.argsort(k, kind="stable")
    assert np.array_equal(k[order], gk) and np.array_equal(res[0][order], mx) and np.array_equal(res[1][order], s) and maps == [None, None]


# ---- 6. deterministic Float64 sums ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint", [1000, 1 << 17])
def test_masked_out_rows_leave_the_fixed_point_window_alone(ch, hint):
    rng = _rng(66)
    ctx = ch.Context(0)
    aggs = [(R.SUM, np.float64, "if"), (R.AVG, np.float64, "if"), (R.SUM, np.float64, "null")]
    modes = ["if", "if", "null"]
    ag = ch.Aggregator(np.uint32, aggs, size_hint=hint, ctx=ctx)
    ref = R.Ref(aggs)
    poison = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300])
    for scale in (1.0, 2.0 ** 40):   # two blocks of different magnitudes
        n = 5000
        keys = rng.integers(0, 30, size=n).astype(np.uint32)
        keys[:4], keys[4:8] = DEAD, LIVE
        # 20 significant bits over ten binades: every kept value is exact in the fixed-point window, before and after the second block
        # widens it, while a Float64 accumulator rounds (a sum near 2^57 has an ulp of 16): double states would not equal math.fsum
        x = rng.integers(1 << 19, 1 << 20, size=n) * 2.0 ** (rng.integers(0, 10, size=n) - 19) * rng.choice(np.array([-1.0, 1.0]), size=n) * scale
        reach = (rng.random(n) < 0.5).astype(np.uint8)
        reach[keys == 3] = 0   # one more group without a kept row: +0.0
        bad = np.flatnonzero(reach == 0)
        x[bad] = poison[rng.integers(0, len(poison), size=len(bad))]
        conds = _special(keys, [reach * 255, reach, (1 - reach).astype(np.uint8)], modes)
        x[keys == LIVE] = 0.5 * scale
        x[keys == DEAD] = poison[:4]
        _assert_special_groups([(keys, conds, None)], modes)
        ag.execute_on_block(keys, [x, x, x], conds=conds)
        ref.add_block(keys, [x, x, x], conds=conds)
    got = ag.convert_to_block(null_maps=True)
    _compare(got, ref)
    k, res, maps = got
    at = {int(v): i for i, v in enumerate(k.tolist())}
    assert res[0][at[3]].tobytes() == np.float64(0.0).tobytes() and res[2][at[DEAD]].tobytes() == np.float64(0.0).tobytes() and maps[2][at[DEAD]] == 1
    # the window still resolves 0.5 beside 2^41: one widened by a masked-out 1e300 would have lost both blocks
    assert res[0][at[LIVE]] == math.fsum([0.5] * 4 + [0.5 * 2.0 ** 40] * 4)


# ---- 7. blocks, merges, states -------------------------------------------------------------------------------------------------------
def test_blocks_merges_and_state_exports_agree(ch):
    rng = _rng(70)
    ctx = ch.Context(0)
    aggs = [(R.SUM, np.int64, "null"), (R.MIN, np.int32, "if"), (R.MAX, np.int32, "null"), (R.AVG, np.uint32, "if"), (R.COUNT, None, "null"), (R.ANY, np.int64, "if"),
            (R.SUM, np.float64, "if")]
    modes = [m for _, _, m in aggs]
    blocks = []
    for b in range(3):
        n = 4000 + 77 * b
        keys = rng.integers(0, 300, size=n).astype(np.uint64)
        keys[:3], keys[3:6] = DEAD, LIVE
        if b == 2:
            keys[6:12] = 999_000   # a group only block 2 has, reached by masked-out rows alone
        a, i32, u32 = rng.integers(-(1 << 60), 1 << 60, size=n), _values(rng, np.int32, n), _values(rng, np.uint32, n)
        f = _values(rng, np.float64, n)
        c1 = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=n)
        nm = (rng.random(n) < 0.5).astype(np.uint8)
        c1[keys == 999_000], nm[keys == 999_000] = 0, 1
        conds = _special(keys, [nm, c1, nm, c1, nm, c1, c1], modes)
        blocks.append((keys, [a, i32, i32, u32, None, a, f], conds))
    _assert_special_groups([(k, c, None) for k, _, c in blocks], modes)
    ref = R.Ref(aggs)
    for k, args, conds in blocks:
        ref.add_block(k, args, conds=conds)

    def fresh():
        return ch.Aggregator(np.uint64, aggs, ctx=ctx)

    def feed(ag, which):
        for k, args, conds in (blocks[i] for i in which):
            ag.execute_on_block(k, args, conds=conds)
        return ag

    one = feed(fresh(), [0, 1, 2])
    _compare(one.convert_to_block(null_maps=True), ref)
    assert one.n_words == 2 + 2 + 2 + 2 + 1 + 2 + 1
    # chgpu_agg_merge: key 999000 exists in the source alone
    dst, src = feed(fresh(), [0, 1]), feed(fresh(), [2])
    dst.merge(src)
    _compare(dst.convert_to_block(null_maps=True), ref)
    # export_state_columns -> merge_states into a fresh aggregator: the seen words travel
    parts = [feed(fresh(), [0]), feed(fresh(), [1, 2])]
    into = fresh()
    for p in parts:
        kc, words, rows = p.export_state_columns()
        assert len(words) == p.n_words
        into.merge_states(kc, words, rows)
    _compare(into.convert_to_block(null_maps=True), ref)
    # the two-level export
    into2 = fresh()
    for p in parts:
        kc, words, rows, counts = p.export_state_columns_two_level()
        assert sum(counts) == rows
        into2.merge_states(kc, words, rows)
    _compare(into2.convert_to_block(null_maps=True), ref)


# ---- 8. limits -----------------------------------------------------------------------------------------------------------------------
def test_limits_count_masked_out_rows_and_the_overflow_row_follows_the_conditions(ch):
    ctx = ch.Context(0)
    aggs = [(R.COUNT, None, "if"), (R.MIN, np.int64, "if"), (R.SUM, np.int64, "null"), (R.MAX, np.int64, "null"), (R.SUM, np.int64, "if")]
    modes = [m for _, _, m in aggs]
    M = 10
    # block 1: 12 keys (0, DEAD, LIVE and 9 more); most of their rows are masked out, yet every key counts towards the limit
    k1 = np.array([0, DEAD, LIVE] + list(range(1, 10)), dtype=np.uint32).repeat(2)
    v1 = np.arange(len(k1), dtype=np.int64) - 7
    c1 = np.zeros(len(k1), dtype=np.uint8)
    c1[::6] = 1
    nm1 = np.ones(len(k1), dtype=np.uint8)
    nm1[1::6] = 0
    conds1 = _special(k1, [c1, c1, nm1, nm1, c1], modes)
    # block 2 runs find-only: rows of absent keys (100 ..) reach the overflow row under their conditions; no absent row reaches the min
    k2 = np.array([0, 100, 101, 102, 3, 103, DEAD, LIVE], dtype=np.uint32)
    v2 = np.array([5, -50, 60, 70, 8, I64_MIN, 1, 2], dtype=np.int64)
    c_cnt = np.array([1, 1, 0, 2, 1, 0, 0, 1], dtype=np.uint8)
    c_min = np.array([1, 0, 0, 0, 1, 0, 0, 1], dtype=np.uint8)
    nm = np.array([0, 1, 1, 1, 0, 1, 1, 0], dtype=np.uint8)       # every absent row is NULL: the overflow row's NULL-mode results are NULL
    conds2 = [c_cnt, c_min, nm, nm, c_cnt]
    _assert_special_groups([(k1, conds1, None), (k2, conds2, None)], modes)
    ag = ch.Aggregator(np.uint32, aggs, ctx=ctx, max_rows_to_group_by=M, group_by_overflow_mode="any", overflow_row=True)
    ref = R.Ref(aggs)
    assert ag.execute_on_block(k1, [None, v1, v1, v1, v1], conds=conds1) is True
    ref.add_block(k1, [None, v1, v1, v1, v1], conds=conds1, overflow_row=True)
    assert len(ag) == 12 and ag.no_more_keys   # masked-out rows of new keys counted: 12 > 10
    assert ag.execute_on_block(k2, [None, v2, v2, v2, v2], conds=conds2) is True
    ref.add_block(k2, [None, v2, v2, v2, v2], conds=conds2, find_only=True, overflow_row=True)
    assert len(ag) == 12
    _compare(ag.convert_to_block(null_maps=True), ref)
    cols, flags = ag.overflow_row(final=True, null_maps=True)
    want, want_flags = ref.overflow_columns()
    got = [c.numpy() for c in cols]
    for j in range(len(aggs)):
        assert got[j].dtype == want[j].dtype and got[j].tobytes() == want[j].tobytes(), (j, got[j], want[j])
        assert (flags[j] is None and want_flags[j] is None) or flags[j].tobytes() == want_flags[j].tobytes(), j
    assert got[0][0] == 2 and got[1][0] == 0 and got[4][0] == 20   # countIf: rows 100, 102; minIf: empty -> 0; sumIf: -50 + 70
    assert flags[2][0] == 1 and flags[3][0] == 1 and got[3][0] == 0
    blocks, maps = ag.convert_to_blocks(final=True, null_maps=True)
    assert blocks[0].is_overflows and maps[0][2][0] == 1 and not blocks[1].is_overflows and blocks[1].rows == 12


# ---- 9. without a key ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["if", "null"])
@pytest.mark.parametrize("dtype", ["int64", "float64", "int8"])
def test_without_key_every_kind(ch, mode, dtype):
    ctx = ch.Context(0)
    rng = _rng(90)
    for kinds in (FIVE, THREE):   # (all eight in NULL mode would need 17 state words)
        aggs = [(k, (dtype, "int32") if k in (R.ARG_MIN, R.ARG_MAX) else None if k == R.COUNT else dtype, mode) for k in kinds]
        ag = ch.Aggregator(None, aggs, ctx=ctx)
        ref = R.Ref(aggs)
        n = 5000
        for b in range(3):
            x, v = _values(rng, dtype, n), rng.integers(-4, 5, size=n).astype(np.int32)
            reach = np.zeros(n, dtype=np.uint8)
            if b == 1:
                reach[3777] = 1          # after a block where everything is masked out: one row passes
            if b == 2:
                reach = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=n)
            c = reach if mode == "if" else (reach == 0).astype(np.uint8)
            where = (rng.random(n) < 0.7).astype(np.uint8) if b == 2 else None
            args = [(x, v) if k in (R.ARG_MIN, R.ARG_MAX) else None if k == R.COUNT else x for k in kinds]
            ag.execute_on_block(None, args, conds=[c] * len(kinds), filter=where)
            ref.add_block(None, args, conds=[c] * len(kinds), where=where)
            _compare(ag.convert_to_block(null_maps=True), ref)


def test_without_key_emptiness_is_per_function(ch):
    ctx = ch.Context(0)
    aggs = [(R.MAX, np.int64, "if"), (R.MAX, np.int64, "if"), (R.MIN, np.int64, "null"), (R.ANY, np.int64, "if"), (R.MAX, np.int64), (R.COUNT, None)]
    x = np.array([-9, -4, -7], dtype=np.int64)
    some, none = np.array([0, 2, 0], dtype=np.uint8), np.zeros(3, dtype=np.uint8)
    conds = [some, none, np.ones(3, dtype=np.uint8), none, None, None]
    ag = ch.Aggregator(None, aggs, ctx=ctx)
    ag.execute_on_block(None, [x, x, x, x, x, None], conds=conds)
    ref = R.Ref(aggs)
    ref.add_block(None, [x, x, x, x, x, None], conds=conds)
    got = ag.convert_to_block(null_maps=True)
    _compare(got, ref)
    _, res, maps = got
    assert [int(r[0]) for r in res] == [-4, 0, 0, 0, -4, 3] and maps[2][0] == 1


# ---- 10. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors(ch):
    K = ch._capi
    ctx = ch.Context(0)
    keys = np.arange(10, dtype=np.uint32)
    v = np.arange(10, dtype=np.int64)
    c = np.ones(10, dtype=np.uint8)

    def code(fn):
        with pytest.raises(K.ChgpuError) as e:
            fn()
        return e.value.code

    ag = ch.Aggregator(np.uint32, [(R.SUM, np.int64, "if"), (R.COUNT, None)], ctx=ctx)
    assert code(lambda: ag.execute_on_block(keys, [v, None], conds=[c.astype(np.uint32), None])) == K.ERR_BAD_ARGUMENTS   # wrong type
    assert code(lambda: ag.execute_on_block(keys, [v, None], conds=[c[:9], None])) == K.ERR_SIZES_MISMATCH               # short column
    assert code(lambda: ag.execute_on_block(keys, [v, None], conds=[None, None])) == K.ERR_BAD_ARGUMENTS                 # missing column
    # the old add calls on a conditioned aggregator
    kc, vc = ctx.upload(keys), ctx.upload(v)
    ptrs = (C.c_void_p * 2)(vc._h, None)
    assert K.lib().chgpu_agg_add_block(ag._h, kc._h, ptrs, 0, 10) == K.ERR_BAD_ARGUMENTS
    assert K.lib().chgpu_agg_add_block_filtered(ag._h, kc._h, ptrs, 0, 10, ctx.upload(c)._h) == K.ERR_BAD_ARGUMENTS
    nmk, keep = C.c_int(0), C.c_int(1)
    assert K.lib().chgpu_agg_execute_on_block(ag._h, kc._h, ptrs, 0, 10, None, C.byref(nmk), C.byref(keep)) == K.ERR_BAD_ARGUMENTS
    assert len(ag) == 0
    ag.execute_on_block(keys, [v, None], conds=[c, None])
    # conditions set after the first block
    modes = (C.c_int * 2)(K.AGG_COND_NONE, K.AGG_COND_NONE)
    assert K.lib().chgpu_agg_set_conditions(ag._h, modes) == K.ERR_BAD_ARGUMENTS
    plain = ch.Aggregator(np.uint32, [(R.SUM, np.int64), (R.COUNT, None)], ctx=ctx)
    plain.execute_on_block(keys, [v, None])
    assert K.lib().chgpu_agg_set_conditions(plain._h, (C.c_int * 2)(K.AGG_COND_IF, K.AGG_COND_NONE)) == K.ERR_BAD_ARGUMENTS
    bad = ch.Aggregator(np.uint32, [(R.SUM, np.int64), (R.COUNT, None)], ctx=ctx)
    assert K.lib().chgpu_agg_set_conditions(bad._h, (C.c_int * 2)(7, 0)) == K.ERR_BAD_ARGUMENTS
    # the new call on an aggregator without conditions works with cond_cols == NULL
    assert K.lib().chgpu_agg_execute_on_block_conditional(bad._h, kc._h, ptrs, None, 0, 10, None, None, None) == K.OK
    assert len(bad) == 10
    # too many words: eight conditioned min / max need 16 words, a ninth word does not fit
    assert ch.Aggregator(np.uint32, [(R.MIN, np.int64, "if")] * 8, ctx=ctx).n_words == 16
    assert code(lambda: ch.Aggregator(np.uint32, [(R.MIN, np.int64, "if")] * 7 + [(R.ARG_MAX, (np.int64, np.int64), "if")], ctx=ctx)) == K.ERR_BAD_ARGUMENTS
    # chgpu_agg_finalize would lose the null map of a NULL-mode sum (count alone is fine)
    nul = ch.Aggregator(np.uint32, [(R.SUM, np.int64, "null")], ctx=ctx)
    nul.execute_on_block(keys, [v], conds=[c])
    assert code(nul.convert_to_block) == K.ERR_BAD_ARGUMENTS
    cnt = ch.Aggregator(np.uint32, [(R.COUNT, None, "null"), (R.MIN, np.int64, "if")], ctx=ctx)
    cnt.execute_on_block(keys, [None, v], conds=[c, 1 - c])
    k, res = cnt.convert_to_block()
    assert res[0].tolist() == [0] * 10 and res[1].tolist() == [0] * 10   # defaults applied: a min over no rows is 0, not INT64_MIN


# ---- 11. the C++ shim ----------------------------------------------------------------------------------------------------------------
def test_cpp_shim_conditions_driver(tmp_path):
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(repo, "clickhouse_amd")
    if not os.path.exists(os.path.join(lib, "libchgpu.so")):
        import __graft_entry__ as g
        g.build()
    exe = str(tmp_path / "agg_conditions_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(repo, "tests", "agg_conditions_driver.cpp"), "-L" + lib, "-lchgpu", "-lpthread",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "agg_conditions_driver OK" in r.stdout
