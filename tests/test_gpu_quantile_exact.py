"""quantileExact / quantilesExact / medianExact (and Low / High) under GROUP BY on the device (clickhouse_amd/csrc/quantile_kernels.hip)
against tests/quantile_exact_ref.py.

Every answer is compared to the reference exactly: as bits, zeros numerically (the reference's order does not tell -0.0 from +0.0).
Where a case claims a path (segments sorted in LDS, segments selected by histogram passes, groups reused from an earlier call) it reads
the `debug` option's `quantile plan=` lines, so that it cannot pass by another route."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantile_exact_ref as R  # noqa: E402
from quantile_exact_ref import QT_CHUNK, QT_SMALL_MAX, QuantileExactRef, bits  # noqa: E402

pytestmark = pytest.mark.gpu

KEY_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
VALUE_DTYPES = R.DTYPES
L3 = [0.5, 0.9, 0.99]


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    c = ch.Context(0)
    c.set_option("debug", 1)
    yield c
    c.close()


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _ints(plan):
    out = {}
    for k, v in plan.items():
        out[k] = v if k == "plan" else tuple(int(x) for x in v.split("->")) if "->" in v else int(v)
    return out


def _plans(err):
    got = [ln[len("chgpu: quantile "):] for ln in err.splitlines() if ln.startswith("chgpu: quantile plan=")]
    return [_ints(dict(kv.split("=", 1) for kv in ln.split() if "=" in kv)) for ln in got]


def _add(q, capfd, keys, values, **kw):
    """add_block -> the call's plan line"""
    capfd.readouterr()
    q.add_block(keys, values, **kw)
    plans = _plans(capfd.readouterr().err)
    assert len(plans) == 1 and plans[0]["plan"] == "add", plans
    return plans[0]


def _finalize(q, capfd, levels, kind="exact"):
    capfd.readouterr()
    k, cols = q.finalize(levels, kind)
    plans = _plans(capfd.readouterr().err)
    assert len(plans) == 1 and plans[0]["plan"] == "finalize", plans
    return k, cols, plans[0]


def _check(q, ref, capfd, levels, kind="exact"):
    """finalize equals the reference for every key, each key once; -> the plan line"""
    k, cols, plan = _finalize(q, capfd, levels, kind)
    want = ref.finalize(levels, kind)
    assert len(cols) == len(np.atleast_1d(levels)) and plan["levels"] == len(cols)
    if ref.key_dtype is None:
        assert k is None and all(len(c) == 1 for c in cols)
        got = np.array([c[0] for c in cols], dtype=ref.value_dtype)
        assert all(c.dtype == ref.value_dtype for c in cols)
        assert R.same(got, np.array(want[None], dtype=ref.value_dtype)), (got, want[None])
        return plan
    assert k.dtype == ref.key_dtype
    kb = bits(k).tolist()
    assert len(set(kb)) == len(kb), "a key was finalised twice"
    assert sorted(kb) == sorted(want), "a group was lost or invented"
    assert plan["groups"] == len(kb) and plan["values"] == len(ref)
    for i, c in enumerate(cols):
        assert c.dtype == ref.value_dtype and len(c) == len(kb)
        w = np.array([want[x][i] for x in kb], dtype=ref.value_dtype)
        bad = np.flatnonzero(~((bits(c) == bits(w)) | ((c == 0) & (w == 0))))
        assert len(bad) == 0, (i, kind, [(kb[j], c[j], w[j]) for j in bad[:5]])
    return plan


def _check_classes(plan, ref):
    small, large, units = ref.classes()
    assert (plan["small"], plan["large"], plan["units"]) == (small, large, units)
    assert plan["passes"] == (0 if large == 0 else ref.value_dtype.itemsize)


def _edges(dtype):
    """the type's minimum and maximum; floats: +-inf, denormals, both zeros, the largest finite values"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        f = np.finfo(dtype)
        return np.array([-np.inf, np.inf, f.min, f.max, f.tiny / 2, -f.tiny / 2, f.smallest_subnormal, -0.0, 0.0, 0.0, -0.0], dtype=dtype)
    i = np.iinfo(dtype)
    return np.array([i.min, i.max, i.min, i.max, 0], dtype=dtype)


def _random_values(rng, dtype, n):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, size=n)).astype(dtype)
    i = np.iinfo(dtype)
    return rng.integers(i.min, i.max, size=n, dtype=dtype, endpoint=True)


# ---- type matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vd", VALUE_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kd", KEY_DTYPES + [None], ids=lambda d: "nokey" if d is None else np.dtype(d).name)
def test_type_matrix(ch, ctx, capfd, kd, vd):
    rng = _rng(300 + np.dtype(vd).num * 31 + (0 if kd is None else np.dtype(kd).num))
    n = 6000
    values = _random_values(rng, vd, n)
    edges = _edges(vd)
    if kd is None:
        keys = None
        values[:len(edges)] = edges
    else:
        ki = np.iinfo(kd)
        kpool = np.concatenate([rng.integers(ki.min, ki.max, size=30, dtype=kd, endpoint=True), np.array([ki.min, ki.max, 0], dtype=kd)])
        keys = kpool[rng.integers(0, len(kpool), size=n)]
        keys[:2500] = kpool[-2]                    # one large segment beside the small ones; it holds every edge value
        keys[2500:2500 + len(edges)] = kpool[-1]   # and so does one small group: both zeros, +-inf and denormals together
        values[:len(edges)] = edges
        values[2500:2500 + len(edges)] = edges
    n_nan = 0
    if np.dtype(vd).kind == "f":
        nan_at = rng.choice(np.arange(len(edges), n), size=37, replace=False)
        values[nan_at] = np.nan
        values[nan_at[:5]] = -np.nan
        n_nan = 37
    ref = QuantileExactRef(kd, vd).add(keys, values)
    q = ch.QuantileExact(kd, vd, ctx=ctx)
    try:
        plan = _add(q, capfd, keys, values)
        assert plan["n"] == n and plan["nan"] == n_nan == ref.nan and plan["entered"] == n - n_nan and plan["held"] == (0, n - n_nan) and plan["rc"] == 0
        assert len(q) == len(ref)
        first = True
        for kind in R.KINDS:
            for levels in ([0.5], [0.0, 0.5, 1.0], [0.29]):
                plan = _check(q, ref, capfd, levels, kind)
                assert plan["cached"] == (0 if first else 1)
                first = False
        _check_classes(plan, ref)
        assert plan["large"] == 1
        if np.dtype(vd) == np.uint64:
            assert (values > np.uint64(2**63)).any()
        k, v = q.export_pairs()
        kb = bits(k).tolist() if k is not None else [0] * len(v)
        assert sorted(zip(kb, bits(v).tolist())) == ref.pairs()
    finally:
        q.close()


def test_float_keys_are_not_implemented(ch, ctx):
    for kd in (np.float32, np.float64):
        with pytest.raises(ch.ChgpuError) as e:
            ch.QuantileExact(kd, np.int64, ctx=ctx)
        assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED


# ---- segment sizes ----------------------------------------------------------------------------------------------------------------
EDGE_SIZES = [1, 2, 63, 64, 65, QT_SMALL_MAX - 1, QT_SMALL_MAX, QT_SMALL_MAX + 1, QT_CHUNK - 1, QT_CHUNK, QT_CHUNK + 1, 3 * QT_CHUNK + 1]


@pytest.mark.parametrize("vd", [np.int64, np.float32, np.uint16], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_segment_sizes_at_the_edges_are_neighbours_in_one_operator(ch, ctx, capfd, vd, order):
    rng = _rng(41 + np.dtype(vd).num)
    # sizes twice, the second time reversed, so that every size has a small and a large neighbour somewhere
    sizes = EDGE_SIZES + EDGE_SIZES[::-1]
    keys = np.repeat(np.arange(len(sizes), dtype=np.uint32) * np.uint32(2654435761), sizes)
    values = _random_values(rng, vd, len(keys))
    if order == "shuffled":
        p = rng.permutation(len(keys))
        keys, values = keys[p], values[p]
    ref = QuantileExactRef(np.uint32, vd).add(keys, values)
    q = ch.QuantileExact(np.uint32, vd, ctx=ctx)
    try:
        _add(q, capfd, keys, values)
        plan = _check(q, ref, capfd, [0.0, 0.5, 1.0, 0.29])
        _check_classes(plan, ref)
        assert plan["small"] == 2 * 7 and plan["large"] == 2 * 5 and plan["units"] == 2 * (1 + 1 + 1 + 2 + 4)
        for kind in ("low", "high"):
            _check(q, ref, capfd, [0.5, 0.57], kind)
    finally:
        q.close()


# ---- the radix select -------------------------------------------------------------------------------------------------------------
def _from_words(words, dtype):
    dtype = np.dtype(dtype)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[dtype.itemsize]
    return np.asarray(words, dtype=np.uint64).astype(u).view(dtype)


def _radix_cases(rng, dtype, n):
    """{name: (values, levels)}: every case one large segment"""
    dtype = np.dtype(dtype)
    w = dtype.itemsize
    base = {1: 0x35, 2: 0x3C35, 4: 0x3F8C5535, 8: 0x3FF12345678C5535}[w]   # (a positive, finite float where dtype is one)
    mid = (w // 2) * 8
    std = [0.0, 0.5, 1.0]
    lo = _from_words(np.full(n, base, dtype=np.uint64) & ~np.uint64(0xFF) | rng.integers(0, 256, size=n, dtype=np.uint64), dtype)
    top_words = np.full(n, base & ((1 << (8 * (w - 1))) - 1), dtype=np.uint64) | (rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(8 * (w - 1)))
    top = _from_words(top_words, dtype)
    if dtype.kind == "f":
        top = top[~np.isnan(top)]
        top = np.concatenate([top, top[:n - len(top)]])
    two = _from_words(np.where(np.arange(n) % 2 == 0, base, base ^ (1 << mid)).astype(np.uint64), dtype)
    h = n // 2
    boundary = [(h - 1 + 0.5) / n, (h + 0.5) / n, (h + 1 + 0.5) / n, (h - 2 + 0.5) / n]
    mixed = _random_values(rng, dtype, n)
    if dtype.kind != "u":
        assert (mixed < 0).any() and (mixed > 0).any()
    return {
        "all_equal": (_from_words(np.full(n, base, dtype=np.uint64), dtype), std),
        "lowest_byte": (lo, std),
        "top_byte": (top, std),
        "two_values": (rng.permutation(two), std + boundary),
        "mixed_signs": (mixed, std),
        "sixteen_same": (mixed, [0.5] * 16),
        "sixteen_distinct": (mixed, [i / 15 for i in range(16)]),
    }


@pytest.mark.parametrize("vd", [np.int64, np.float64, np.uint32, np.float32, np.int16, np.uint8, np.int8], ids=lambda d: np.dtype(d).name)
def test_radix_select_where_it_can_go_wrong(ch, ctx, capfd, vd):
    rng = _rng(77 + np.dtype(vd).num)
    n = 2 * QT_CHUNK + 1000   # three work units, the last one short
    for name, (values, levels) in _radix_cases(rng, vd, n).items():
        assert len(values) == n
        # a small group on either side of the large one
        keys = np.concatenate([np.full(3, 1, dtype=np.uint16), np.full(n, 2, dtype=np.uint16), np.full(5, 3, dtype=np.uint16)])
        vals = np.concatenate([values[:3], values, values[:5]])
        ref = QuantileExactRef(np.uint16, vd).add(keys, vals)
        q = ch.QuantileExact(np.uint16, vd, ctx=ctx)
        try:
            q.add_block(keys, vals)
            plan = _check(q, ref, capfd, levels)
            assert (plan["small"], plan["large"], plan["units"], plan["passes"]) == (2, 1, 3, np.dtype(vd).itemsize), name
            if name == "two_values":
                r = [R.rank("exact", l, n) for l in levels]
                assert r[3:] == [n // 2 - 1, n // 2, n // 2 + 1, n // 2 - 2]
                _check(q, ref, capfd, [0.5], "low")
                _check(q, ref, capfd, [0.5], "high")
        finally:
            q.close()
        # and as the one segment of an operator without key (the store itself is the segment)
        q = ch.QuantileExact(None, vd, ctx=ctx)
        try:
            q.add_block(None, values)
            plan = _check(q, QuantileExactRef(None, vd).add(None, values), capfd, levels)
            assert (plan["small"], plan["large"], plan["groups"]) == (0, 1, 1), name
        finally:
            q.close()


# ---- many groups, skew --------------------------------------------------------------------------------------------------------------
def test_many_tiny_groups(ch, ctx, capfd):
    rng = _rng(5)
    groups = 200_000
    sizes = rng.integers(1, 4, size=groups)
    keys = np.repeat(rng.permutation(np.arange(groups, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)), sizes)
    p = rng.permutation(len(keys))
    keys = keys[p]
    values = rng.standard_normal(len(keys))
    ref = QuantileExactRef(np.uint64, np.float64).add(keys, values)
    q = ch.QuantileExact(np.uint64, np.float64, ctx=ctx)
    try:
        _add(q, capfd, keys, values)
        plan = _check(q, ref, capfd, L3)
        assert (plan["groups"], plan["small"], plan["large"], plan["units"], plan["passes"]) == (groups, groups, 0, 0, 0)
        _check(q, ref, capfd, [0.5], "low")
    finally:
        q.close()


@pytest.mark.parametrize("order", ["random", "sorted"])
def test_one_heavy_group_among_thousands(ch, ctx, capfd, order):
    rng = _rng(6)
    light = 5000
    sizes = rng.integers(1, 4, size=light)
    keys = np.concatenate([np.repeat(np.arange(1, light + 1, dtype=np.uint32), sizes), np.full(100_000, 2500, dtype=np.uint32)])
    values = rng.integers(-10**12, 10**12, size=len(keys), dtype=np.int64)
    p = rng.permutation(len(keys)) if order == "random" else np.argsort(keys, kind="stable")
    keys, values = keys[p], values[p]
    ref = QuantileExactRef(np.uint32, np.int64).add(keys, values)
    q = ch.QuantileExact(np.uint32, np.int64, ctx=ctx)
    try:
        _add(q, capfd, keys, values)
        plan = _check(q, ref, capfd, L3)
        assert (plan["groups"], plan["small"], plan["large"]) == (light, light - 1, 1)
        _check_classes(plan, ref)
    finally:
        q.close()


# ---- blocks -------------------------------------------------------------------------------------------------------------------------
def test_blocks_with_ranges_and_a_filter_and_finalize_between_them(ch, ctx, capfd):
    rng = _rng(8)
    n = 9000
    keys = rng.integers(0, 50, size=n, dtype=np.int32) - 25
    keys[rng.random(n) < 0.4] = 7                     # key 7 grows from small to large over the blocks
    values = rng.standard_normal(n).astype(np.float32)
    values[rng.random(n) < 0.05] = np.nan
    filt = (rng.integers(0, 4, size=n) != 0).astype(np.uint8) * np.uint8(3)
    ref = QuantileExactRef(np.int32, np.float32)
    q = ch.QuantileExact(np.int32, np.float32, ctx=ctx)
    kcol, vcol, fcol = ctx.upload(keys), ctx.upload(values), ctx.upload(filt)
    try:
        larges = []
        for (b, e, f) in ((0, 3000, fcol), (3000, 3001, None), (3001, 9000, fcol)):
            fnp = None if f is None else filt
            ref.add(keys, values, b, e, filter=fnp)
            plan = _add(q, capfd, kcol, vcol, row_begin=b, row_end=e, filter=f)
            assert plan["n"] == e - b and plan["nan"] == ref.nan and plan["held"][1] == len(ref) == len(q)
            plan = _check(q, ref, capfd, L3)
            assert plan["cached"] == 0                                # the groups of the call before were dropped
            assert _check(q, ref, capfd, [0.1], "high")["cached"] == 1
            _check_classes(plan, ref)
            larges.append(plan["large"])
        assert larges == [0, 0, 1]
        # a block none of whose rows enters changes nothing and keeps the groups
        plan = _add(q, capfd, kcol, vcol, filter=np.zeros(n, dtype=np.uint8))
        assert plan["entered"] == 0 and plan["held"] == (len(ref), len(ref))
        assert _check(q, ref, capfd, L3)["cached"] == 1
        plan = _add(q, capfd, kcol, vcol, row_begin=5, row_end=5)
        assert plan["n"] == 0 and _check(q, ref, capfd, L3)["cached"] == 1
    finally:
        q.close()


def test_merge_equals_one_operator_fed_both_inputs_and_export_feeds_a_fresh_one(ch, ctx, capfd):
    rng = _rng(9)
    k1, k2 = rng.integers(0, 300, size=7000, dtype=np.uint16), rng.integers(200, 500, size=5000, dtype=np.uint16)
    k2[:3000] = 250
    v1, v2 = rng.integers(-5000, 5000, size=7000, dtype=np.int16), rng.integers(-5000, 5000, size=5000, dtype=np.int16)
    a, b, fresh = (ch.QuantileExact(np.uint16, np.int16, ctx=ctx) for _ in range(3))
    try:
        a.add_block(k1, v1)
        b.add_block(k2, v2)
        ref_b = QuantileExactRef(np.uint16, np.int16).add(k2, v2)
        ref = QuantileExactRef(np.uint16, np.int16).add(k1, v1)
        _check(a, ref, capfd, L3)
        capfd.readouterr()
        a.merge(b)
        plan = _plans(capfd.readouterr().err)[0]
        assert plan["plan"] == "merge" and plan["n"] == 5000 and plan["held"] == (7000, 12000)
        ref.merge(ref_b)
        assert _check(a, ref, capfd, L3)["cached"] == 0
        _check(b, ref_b, capfd, L3)                           # src stays valid
        k, v = a.export_pairs()
        assert k.dtype == np.uint16 and v.dtype == np.int16
        assert sorted(zip(bits(k).tolist(), bits(v).tolist())) == ref.pairs()
        ek, ev = a.export_pairs_columns()
        fresh.add_block(ek, ev)                               # the pairs, still in HBM, into a peer
        _check(fresh, ref, capfd, [0.0, 0.25, 0.5, 1.0], "high")
        a.merge(a)                                            # a multiset union with itself doubles every value
        ref.merge(QuantileExactRef(np.uint16, np.int16).add(*[np.concatenate(x) for x in ((k1, k2), (v1, v2))]))
        _check(a, ref, capfd, L3, "low")
    finally:
        a.close(), b.close(), fresh.close()


def test_finalize_twice_with_different_levels_and_kinds(ch, ctx, capfd):
    rng = _rng(10)
    keys = rng.integers(0, 9, size=30_000, dtype=np.uint8)
    values = rng.integers(0, 2**64, size=30_000, dtype=np.uint64)
    ref = QuantileExactRef(np.uint8, np.uint64).add(keys, values)
    q = ch.QuantileExact(np.uint8, np.uint64, ctx=ctx)
    try:
        q.add_block(keys, values)
        assert (values > np.uint64(2**63)).any()
        for levels, kind in (([0.5], "exact"), ([0.5], "low"), ([0.5], "high"), ([0.99, 0.01], "exact"), ([1.0] * 16, "low"), ([0.5], "exact")):
            plan = _check(q, ref, capfd, levels, kind)
            assert plan["large"] == 9 and plan["passes"] == 8
    finally:
        q.close()


def test_without_key_one_row_and_the_empty_operator(ch, ctx, capfd):
    for vd in (np.float64, np.float32, np.int32, np.uint8):
        q = ch.QuantileExact(None, vd, ctx=ctx)
        ref = QuantileExactRef(None, vd)
        try:
            k, cols = q.finalize(L3)
            assert k is None and len(q) == 0
            assert R.same(np.concatenate(cols), np.array([R.empty_value(vd)] * 3, dtype=vd))
            values = _random_values(_rng(11), vd, 100)
            plan = _add(q, capfd, None, values, filter=np.zeros(100, dtype=np.uint8))
            assert plan["entered"] == 0
            assert R.same(np.concatenate(q.finalize([0.5])[1]), np.array([R.empty_value(vd)], dtype=vd))
            ref.add(None, values)
            q.add_block(None, values)
            plan = _check(q, ref, capfd, [0.0, 0.29, 0.57, 1.0])
            assert (plan["groups"], plan["small"], plan["large"]) == (1, 1, 0)
        finally:
            q.close()
    # a keyed operator that holds nothing: no rows, and every key looked up gets the empty-state value
    q = ch.QuantileExact(np.uint32, np.float64, ctx=ctx)
    try:
        k, cols = q.finalize(L3)
        assert len(k) == 0 and k.dtype == np.uint32 and [len(c) for c in cols] == [0, 0, 0]
        got = q.quantiles_for_keys(np.arange(5, dtype=np.uint32), [0.5, 0.9])
        assert len(got) == 2 and all(np.isnan(g).all() and len(g) == 5 for g in got)
        ek, ev = q.export_pairs()
        assert len(ek) == 0 and len(ev) == 0
    finally:
        q.close()


def test_for_keys_lines_up_with_an_aggregator_finalize(ch, ctx, capfd):
    rng = _rng(12)
    n = 20_000
    keys = rng.integers(0, 40, size=n, dtype=np.uint32)
    keys[:6000] = 3
    a = rng.integers(-100, 100, size=n, dtype=np.int64)
    x = rng.standard_normal(n)
    cond = (rng.integers(0, 3, size=n) != 0).astype(np.uint8)
    cond[keys == 17] = 0                           # every row of key 17 is masked out of the quantile
    agg = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)], ctx=ctx)
    q = ch.QuantileExact(np.uint32, np.float64, ctx=ctx)
    qi = ch.QuantileExact(np.uint32, np.int64, ctx=ctx)
    try:
        agg.execute_on_block(keys, [a, None])
        q.add_block(keys, x, filter=cond)
        qi.add_block(keys, a, filter=cond)
        gk, _ = agg.finalize_columns()
        capfd.readouterr()
        got = q.quantiles_for_keys_column(gk, L3)            # the key Column of the aggregator's result, still in HBM
        plan = _plans(capfd.readouterr().err)[0]
        assert plan["plan"] == "for_keys" and plan["large"] == 1 and plan["levels"] == 3
        gkeys = gk.numpy()
        assert sorted(gkeys.tolist()) == sorted(set(keys.tolist()))
        ref = QuantileExactRef(np.uint32, np.float64).add(keys, x, filter=cond)
        want = ref.for_keys(gkeys, L3)
        for g, w in zip(got, want):
            assert R.same(g.numpy(), w)
        assert np.isnan(got[0].numpy()[gkeys == 17]).all() and 17 not in ref.finalize(L3)
        # absent keys and repeated keys, integers: 0 for a key without values
        probe = np.concatenate([gkeys, gkeys[:7], np.array([17, 4000, 17, 2**32 - 1], dtype=np.uint32)])
        refi = QuantileExactRef(np.uint32, np.int64).add(keys, a, filter=cond)
        for kind in R.KINDS:
            for g, w in zip(qi.quantiles_for_keys(probe, [0.5, 1.0], kind), refi.for_keys(probe, [0.5, 1.0], kind)):
                assert R.same(g, w)
        assert qi.quantiles_for_keys(probe, [0.5])[0][-4:].tolist() == [0, 0, 0, 0]
    finally:
        agg.close(), q.close(), qi.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_entry_checks_return_their_codes_and_leave_the_operator_usable(ch, ctx, capfd):
    import ctypes as C
    K = ch._capi
    keys = np.arange(100, dtype=np.uint32)
    values = np.arange(100, dtype=np.int64)
    kcol, vcol = ctx.upload(keys), ctx.upload(values)
    q = ch.QuantileExact(np.uint32, np.int64, ctx=ctx)
    nokey = ch.QuantileExact(None, np.int64, ctx=ctx)
    other = ch.QuantileExact(np.uint32, np.int32, ctx=ctx)

    def code(fn, *a, **kw):
        with pytest.raises(ch.ChgpuError) as e:
            fn(*a, **kw)
        return e.value.code, str(e.value)

    try:
        q.add_block(kcol, vcol)
        for bad in ([-0.1], [1.5], [float("nan")], [0.5, -0.1], [0.5, float("inf")]):
            assert code(q.finalize, bad)[0] == K.ERR_BAD_ARGUMENTS
            assert code(q.quantiles_for_keys, keys, bad)[0] == K.ERR_BAD_ARGUMENTS
        assert code(q.finalize, [])[0] == K.ERR_BAD_ARGUMENTS and code(q.finalize, [0.5] * 17)[0] == K.ERR_BAD_ARGUMENTS
        assert code(q.quantiles_for_keys, keys, [])[0] == K.ERR_BAD_ARGUMENTS and code(q.quantiles_for_keys, keys, [0.5] * 17)[0] == K.ERR_BAD_ARGUMENTS
        for reserved in ("inclusive", "exclusive", "weighted"):
            assert code(q.finalize, [0.5], reserved)[0] == K.ERR_NOT_IMPLEMENTED
            assert code(q.quantiles_for_keys, keys, [0.5], reserved)[0] == K.ERR_NOT_IMPLEMENTED
        assert code(q.finalize, [0.5], 9)[0] == K.ERR_BAD_ARGUMENTS and code(q.finalize, [0.5], -1)[0] == K.ERR_BAD_ARGUMENTS
        assert code(q.add_block, ctx.upload(keys.astype(np.uint64)), vcol)[0] == K.ERR_BAD_ARGUMENTS          # key type
        assert code(q.add_block, kcol, ctx.upload(values.astype(np.int32)))[0] == K.ERR_BAD_ARGUMENTS          # value type
        assert code(q.add_block, kcol, vcol, filter=ctx.upload(np.ones(100, dtype=np.uint16)))[0] == K.ERR_BAD_ARGUMENTS
        assert code(q.add_block, kcol, vcol, row_begin=6, row_end=5)[0] == K.ERR_BAD_ARGUMENTS
        assert code(q.add_block, kcol, vcol, row_begin=0, row_end=101)[0] == K.ERR_BAD_ARGUMENTS
        assert code(q.add_block, ctx.upload(keys[:99]), vcol)[0] == K.ERR_SIZES_MISMATCH
        assert code(q.add_block, kcol, vcol, filter=np.ones(99, dtype=np.uint8))[0] == K.ERR_SIZES_MISMATCH
        c, msg = code(q.add_block, None, vcol)
        assert c == K.ERR_BAD_ARGUMENTS and "NULL" in msg
        assert code(q.merge, other)[0] == K.ERR_BAD_ARGUMENTS and code(q.merge, nokey)[0] == K.ERR_BAD_ARGUMENTS
        assert code(q.quantiles_for_keys, keys.astype(np.uint64), [0.5])[0] == K.ERR_BAD_ARGUMENTS
        assert code(nokey.quantiles_for_keys, keys, [0.5])[0] == K.ERR_BAD_ARGUMENTS
        h = C.c_void_p()
        assert K.lib().chgpu_quantile_create(ctx._h, 77, K.I64, C.byref(h)) == K.ERR_BAD_ARGUMENTS
        assert K.lib().chgpu_quantile_create(ctx._h, K.U32, 77, C.byref(h)) == K.ERR_BAD_ARGUMENTS
        # NULL outputs on a live handle
        n = C.c_uint64(0)
        a, b = C.c_void_p(), C.c_void_p()
        lv = (C.c_double * 1)(0.5)
        res = (C.c_void_p * 1)()
        L = K.lib()
        for rc in (L.chgpu_quantile_size(q._h, None), L.chgpu_quantile_finalize(q._h, 0, 1, lv, None, res, C.byref(n)),
                   L.chgpu_quantile_finalize(q._h, 0, 1, lv, C.byref(a), None, C.byref(n)), L.chgpu_quantile_finalize(q._h, 0, 1, lv, C.byref(a), res, None),
                   L.chgpu_quantile_finalize(q._h, 0, 1, None, C.byref(a), res, C.byref(n)), L.chgpu_quantile_export_pairs(q._h, C.byref(a), C.byref(b), None),
                   L.chgpu_quantile_export_pairs(q._h, None, C.byref(b), C.byref(n)), L.chgpu_quantile_for_keys(q._h, 0, 1, lv, kcol._h, None),
                   L.chgpu_quantile_for_keys(q._h, 0, 1, lv, None, res), L.chgpu_quantile_merge(q._h, None), L.chgpu_quantile_create(ctx._h, K.U32, K.I64, None)):
            assert rc == K.ERR_BAD_ARGUMENTS and b"NULL" in L.chgpu_last_error()
        # without key: keys_out may be NULL
        assert L.chgpu_quantile_finalize(nokey._h, 0, 1, lv, None, res, C.byref(n)) == K.OK and n.value == 1
        L.chgpu_col_free(C.c_void_p(res[0]))
        # nothing above changed the operator
        ref = QuantileExactRef(np.uint32, np.int64).add(keys, values)
        _check(q, ref, capfd, L3)
        assert len(q) == 100
    finally:
        q.close()
        nokey.close()
        other.close()


def _snapshot(q):
    k, v = q.export_pairs()
    return len(q), sorted(zip(bits(k).tolist(), bits(v).tolist()))


def test_a_refused_allocation_leaves_the_operator_as_it_was(ch, capfd):
    c = ch.Context(0)
    try:
        c.set_option("debug", 1)
        rng = _rng(13)
        keys = rng.integers(0, 20, size=30_000, dtype=np.uint32)
        keys[:5000] = 4
        values = rng.standard_normal(30_000)
        ref = QuantileExactRef(np.uint32, np.float64).add(keys[:3000], values[:3000])
        q = ch.QuantileExact(np.uint32, np.float64, ctx=c)
        try:
            q.add_block(keys[:3000], values[:3000])
            before = _snapshot(q)
            assert before == (3000, ref.pairs())
            _check(q, ref, capfd, L3)
            for nth in (1, 2):                               # the store grows by two allocations: keys, values
                c.set_option("test_quantile_fail_alloc", nth)
                capfd.readouterr()
                with pytest.raises(ch.ChgpuError) as e:
                    q.add_block(keys, values)
                assert e.value.code == ch._capi.ERR_OOM
                plan = _plans(capfd.readouterr().err)[0]
                assert plan["rc"] == ch._capi.ERR_OOM and plan["held"] == (3000, 3000) and plan["entered"] == 0
                c.set_option("test_quantile_fail_alloc", 0)
                assert _snapshot(q) == before
                assert _check(q, ref, capfd, L3)["cached"] == 1
            # a refused merge
            other = ch.QuantileExact(np.uint32, np.float64, ctx=c)
            other.add_block(keys, values)
            c.set_option("test_quantile_fail_alloc", 2)
            with pytest.raises(ch.ChgpuError) as e:
                q.merge(other)
            assert e.value.code == ch._capi.ERR_OOM
            c.set_option("test_quantile_fail_alloc", 0)
            assert _snapshot(q) == before
            other.close()
            # a refused finalize, at every allocation it makes; then the same finalize goes through
            q.add_block(keys, values)
            ref.add(keys, values)
            before = _snapshot(q)
            refused = 0
            for nth in range(1, 40):
                c.set_option("test_quantile_fail_alloc", nth)
                try:
                    q.finalize(L3)
                    c.set_option("test_quantile_fail_alloc", 0)
                    break
                except ch.ChgpuError as e:
                    assert e.code == ch._capi.ERR_OOM
                    refused += 1
                c.set_option("test_quantile_fail_alloc", 0)
                assert _snapshot(q) == before
            assert refused >= 10                             # groups, offsets, table, segments, states, histograms, results
            assert _snapshot(q) == before
            _check(q, ref, capfd, L3)
            c.set_option("test_quantile_fail_alloc", 3)
            with pytest.raises(ch.ChgpuError) as e:
                q.quantiles_for_keys(keys[:10], L3)
            assert e.value.code == ch._capi.ERR_OOM
            c.set_option("test_quantile_fail_alloc", 0)
            assert _snapshot(q) == before
            for g, w in zip(q.quantiles_for_keys(keys[:10], L3), ref.for_keys(keys[:10], L3)):
                assert R.same(g, w)
        finally:
            q.close()
    finally:
        c.close()


# ---- levels in batches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vd", [np.float64, np.int16], ids=lambda d: np.dtype(d).name)
def test_levels_run_in_batches_without_showing_in_the_results(ch, capfd, vd):
    """test_quantile_hist_budget lowers the histogram memory of one batch, so that 5 large segments already split 16 levels: batches
    that start past level 0, a shorter last batch, the shared first-pass histogram once per batch.  Same answers as in one batch."""
    c = ch.Context(0)
    try:
        c.set_option("debug", 1)
        rng = _rng(14 + np.dtype(vd).num)
        sizes = [3000, 7, QT_SMALL_MAX + 1, 2 * QT_CHUNK + 5, 1, 2500, 40, 4000]
        keys = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
        values = _random_values(rng, vd, len(keys))
        p = rng.permutation(len(keys))
        keys, values = keys[p], values[p]
        ref = QuantileExactRef(np.uint32, vd).add(keys, values)
        levels = [0.0, 1.0, 0.5, 0.5] + [i / 13 for i in range(1, 13)]
        width = np.dtype(vd).itemsize
        q = ch.QuantileExact(np.uint32, vd, ctx=c)
        try:
            q.add_block(keys, values)
            plan = _check(q, ref, capfd, levels)
            assert (plan["large"], plan["units"], plan["passes"]) == (5, 7, width)              # one batch of 16
            for budget, batches in ((5 * 3 * 1024, 6), (5 * 5 * 1024 + 1023, 4), (1, 16), (5 * 16 * 1024, 1)):
                c.set_option("test_quantile_hist_budget", budget)
                for kind in ("exact", "low"):
                    plan = _check(q, ref, capfd, levels, kind)
                    assert plan["passes"] == width * batches and plan["cached"] == 1, (budget, plan)
                assert _check(q, ref, capfd, levels[:2])["passes"] == width * (2 if budget == 1 else 1)
        finally:
            q.close()
    finally:
        c.close()
