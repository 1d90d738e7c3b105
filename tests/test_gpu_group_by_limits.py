"""max_rows_to_group_by / group_by_overflow_mode / overflow_row on the device, against a numpy model of the reference's semantics
(Aggregator.cpp:1181-1194 find-only rows, :1611 checkLimits after the block, :1816-1830): a block is added in full unless no_more_keys
is set, then every row finds its key and a row whose key the table lacks goes to the overflow row (or is dropped).  Every plan the
selection picks is forced with the existing options and size hints and recognised by its `debug` line; counts and integer sums are
compared bit-exact (mod 2^64)."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _keysets(rng, dtype, n_present, n_new, zero_present):
    """disjoint key sets A (present after block 1) and B (new in block 2); the key 0 in A or in B"""
    hi = min(np.iinfo(dtype).max, 2**62)
    pool = rng.choice(np.arange(1, 256, dtype=np.uint64), size=n_present + n_new - 1, replace=False) if hi < 256 else None
    if pool is None:
        pool = np.unique(rng.integers(1, hi, size=3 * (n_present + n_new), dtype=np.uint64))
        pool = rng.permutation(pool)[: n_present + n_new - 1]
    pool = pool.astype(dtype)
    z = np.zeros(1, dtype=dtype)
    if zero_present:
        return np.concatenate([z, pool[: n_present - 1]]), pool[n_present - 1:]
    return pool[:n_present], np.concatenate([z, pool[n_present:]])


def _model(blocks, M, ovf_on):
    """blocks: [(keys, [arg arrays])] for count + sum per argument -> ({key: [count, sums...]}, overflow [count, sums...] or None)"""
    groups, nmk = {}, False
    n_args = len(blocks[0][1])
    ovf = [0] * (1 + n_args)
    for keys, args in blocks:
        uk, inv = np.unique(keys, return_inverse=True)
        cnt = np.bincount(inv, minlength=len(uk)).astype(np.uint64)
        sums = []
        for a in args:
            s = np.zeros(len(uk), dtype=np.uint64)
            np.add.at(s, inv, a.astype(np.int64).view(np.uint64))
            sums.append(s)
        for x in range(len(uk)):
            k = int(uk[x])
            st = [int(cnt[x])] + [int(s[x]) for s in sums]
            if nmk and k not in groups:
                ovf = [(o + v) & M64 for o, v in zip(ovf, st)]
                continue
            old = groups.setdefault(k, [0] * (1 + n_args))
            groups[k] = [(o + v) & M64 for o, v in zip(old, st)]
        if not nmk and M and len(groups) > M:
            nmk = True
    return groups, (ovf if ovf_on else None)


def _device(ch, ag, n_args):
    keys, res = ag.convert_to_block()
    got = {}
    for i, k in enumerate(keys.tolist()):
        got[int(k)] = [int(np.uint64(res[0][i]))] + [int(np.asarray(res[1 + a][i]).astype(np.int64).view(np.uint64)) for a in range(n_args)]
    ovf = ag.overflow_row(final=True)
    if ovf is not None:
        vals = [c.numpy()[0] for c in ovf]
        ovf = [int(np.uint64(vals[0]))] + [int(np.asarray(vals[1 + a]).astype(np.int64).view(np.uint64)) for a in range(n_args)]
    return got, ovf


def _plan_line(err):
    lines = [ln for ln in err.splitlines() if ln.startswith("chgpu: ") and "GROUP BY" in ln and "finish rounds" not in ln]
    return lines


# plan -> (options, size_hint, rows of block 2, expected plan-line fragment, key dtypes, argument words)
PLANS = {
    "ranged": ({}, 1000, 200_000, "ranged GROUP BY", ["uint8", "uint16", "uint32", "uint64"], 1),
    "rows_lds": ({"tune_agg_no_ranged": 1}, 1000, 200_000, "kernel=rows_lds", ["uint8", "uint16", "uint32", "uint64"], 1),
    "rows_direct": ({}, 1 << 20, 200_000, "kernel=rows_direct", ["uint8", "uint16", "uint32", "uint64"], 1),
    "partitioned": ({"tune_gb_no_tiled": 1}, 1 << 19, 5 << 20, "partitioned GROUP BY", ["uint32", "uint64"], 1),
    "tile_sorted": ({}, 1 << 19, 5 << 20, "tile-sorted GROUP BY", ["uint32", "uint64"], 1),
    "word_passes": ({}, 1 << 19, 5 << 20, "tile-sorted GROUP BY", ["uint32", "uint64"], 2),
}
CASES = [(p, kd, ovf, zp) for p, spec in PLANS.items() for kd in spec[4] for ovf in (True, False) for zp in (True, False)]


@pytest.mark.parametrize("plan,key_dtype,ovf_on,zero_present", CASES)
def test_every_plan_in_find_only_mode(ch, capfd, plan, key_dtype, ovf_on, zero_present):
    opts, hint, n2, frag, _, n_args = PLANS[plan]
    kd = np.dtype(key_dtype)
    rng = _rng(zlib.crc32(f"{plan}-{key_dtype}-{ovf_on}-{zero_present}".encode()))
    n_a = 100 if kd.itemsize == 1 else 500 if hint <= 1000 else 20_000 if kd.itemsize == 2 else 200_000
    A, B = _keysets(rng, kd, n_a, n_a, zero_present)
    k1 = rng.permutation(np.concatenate([A, rng.choice(A, size=4 * len(A))]))
    k2 = rng.permutation(np.concatenate([rng.choice(A, size=n2 // 2), rng.choice(B, size=n2 - n2 // 2)]))
    a1 = [rng.integers(-1000, 1 << 40, size=len(k1), dtype=np.int64) for _ in range(n_args)]
    a2 = [rng.integers(-1000, 1 << 40, size=len(k2), dtype=np.int64) for _ in range(n_args)]
    M = len(A) - 1
    ctx = ch.Context(0)
    for name, value in opts.items():
        ctx.set_option(name, value)
    ctx.set_option("debug", 1)
    aggs = [(ch.AGG_COUNT, None)] + [(ch.AGG_SUM, np.int64)] * n_args
    ag = ch.Aggregator(kd, aggs, size_hint=hint, ctx=ctx, max_rows_to_group_by=M, group_by_overflow_mode="any", overflow_row=ovf_on)
    assert ag.execute_on_block(ctx.upload(k1), [None] + [ctx.upload(a) for a in a1]) is True
    assert ag.no_more_keys
    capfd.readouterr()
    assert ag.execute_on_block(ctx.upload(k2), [None] + [ctx.upload(a) for a in a2]) is True
    err = capfd.readouterr().err
    lines = _plan_line(err)
    assert any(frag in ln for ln in lines), err
    if plan == "word_passes":
        assert sum("tile-sorted GROUP BY" in ln for ln in lines) == 2, err
    assert len(ag) == len(A)
    want, want_ovf = _model([(k1, a1), (k2, a2)], M, ovf_on)
    got, got_ovf = _device(ch, ag, n_args)
    assert got == want
    assert got_ovf == want_ovf


@pytest.mark.parametrize("fused", [True, False])
def test_where_mask_applies_before_find_only(ch, capfd, fused):
    kd = np.dtype(np.uint32)
    rng = _rng(7 + fused)
    A, B = _keysets(rng, kd, 300, 300, True)
    k1 = rng.permutation(np.concatenate([A, A]))
    n2 = 300_000
    k2 = rng.permutation(np.concatenate([rng.choice(A, size=n2 // 2), rng.choice(B, size=n2 - n2 // 2)]))
    a2 = rng.integers(-1000, 1000, size=n2, dtype=np.int64)
    mask = (rng.random(n2) < 0.6).astype(np.uint8)
    ctx = ch.Context(0)
    ctx.set_option("debug", 1)
    hint = 1000 if fused else 1 << 20
    ag = ch.Aggregator(kd, [(ch.AGG_COUNT, None), (ch.AGG_SUM, np.int64)], size_hint=hint, ctx=ctx, max_rows_to_group_by=len(A) - 1,
                       group_by_overflow_mode="any", overflow_row=True)
    ag.execute_on_block(ctx.upload(k1), [None, ctx.upload(np.ones(len(k1), dtype=np.int64))])
    capfd.readouterr()
    ag.execute_on_block(ctx.upload(k2), [None, ctx.upload(a2)], filter=ctx.upload(mask))
    err = capfd.readouterr().err
    assert any(("ranged GROUP BY" if fused else "rows_direct") in ln for ln in _plan_line(err)), err
    keep = mask != 0
    want, want_ovf = _model([(k1, [np.ones(len(k1), dtype=np.int64)]), (k2[keep], [a2[keep]])], len(A) - 1, True)
    got, got_ovf = _device(ch, ag, 1)
    assert got == want and got_ovf == want_ovf


@pytest.mark.parametrize("ovf_on", [True, False])
@pytest.mark.parametrize("key_dtype", ["uint8", "uint16", "uint32", "uint64"])
def test_extremum_plan_in_find_only_mode(ch, capfd, key_dtype, ovf_on):
    kd = np.dtype(key_dtype)
    rng = _rng(11)
    A, B = _keysets(rng, kd, 100, 100, ovf_on)
    k1 = rng.permutation(np.concatenate([A, A]))
    n2 = 100_000
    k2 = rng.permutation(np.concatenate([rng.choice(A, size=n2 // 2), rng.choice(B, size=n2 - n2 // 2)]))
    v1 = rng.integers(-10**9, 10**9, size=len(k1), dtype=np.int64)
    v2 = rng.integers(-10**9, 10**9, size=n2, dtype=np.int64)
    ctx = ch.Context(0)
    ctx.set_option("debug", 1)
    ag = ch.Aggregator(kd, [(ch.AGG_MIN, np.int64), (ch.AGG_MAX, np.int64), (ch.AGG_ANY, np.int64)], ctx=ctx, max_rows_to_group_by=len(A) - 1,
                       group_by_overflow_mode="any", overflow_row=ovf_on)
    ag.execute_on_block(ctx.upload(k1), [ctx.upload(v1)] * 3)
    capfd.readouterr()
    ag.execute_on_block(ctx.upload(k2), [ctx.upload(v2)] * 3)
    assert "states=extremum" in capfd.readouterr().err
    keys, res = ag.convert_to_block()
    allk, allv = np.concatenate([k1, k2]), np.concatenate([v1, v2])
    inA = np.isin(allk, A)
    for i, k in enumerate(keys.tolist()):
        sel = allv[inA & (allk == k)]
        assert (res[0][i], res[1][i], res[2][i]) == (sel.min(), sel.max(), sel[0])
    if not ovf_on:
        assert ag.overflow_row() is None
        return
    miss = v2[~np.isin(k2, A)]
    o = [c.numpy()[0] for c in ag.overflow_row()]
    assert (o[0], o[1], o[2]) == (miss.min(), miss.max(), miss[0])


def test_limit_boundary_and_the_crossing_block(ch):
    ctx = ch.Context(0)
    ag = ch.Aggregator(np.uint64, [(ch.AGG_COUNT, None)], ctx=ctx, max_rows_to_group_by=10, group_by_overflow_mode="any")
    assert ag.execute_on_block(ctx.upload(np.arange(10, dtype=np.uint64)), [None])
    assert not ag.no_more_keys and len(ag) == 10            # G == M: no trigger
    ag.execute_on_block(ctx.upload(np.arange(5, 25, dtype=np.uint64)), [None])
    assert ag.no_more_keys and len(ag) == 25                # the crossing block is present in full
    ag.execute_on_block(ctx.upload(np.arange(20, 40, dtype=np.uint64)), [None])
    assert len(ag) == 25


def test_throw_mode(ch):
    from clickhouse_amd import _capi as K
    ctx = ch.Context(0)
    ag = ch.Aggregator(np.uint32, [(ch.AGG_COUNT, None)], ctx=ctx, max_rows_to_group_by=10, group_by_overflow_mode="throw")
    ag.execute_on_block(ctx.upload(np.arange(10, dtype=np.uint32)), [None])
    with pytest.raises(K.ChgpuError) as e:
        ag.execute_on_block(ctx.upload(np.arange(11, dtype=np.uint32)), [None])
    assert e.value.code == K.ERR_TOO_MANY_ROWS
    assert str(e.value).endswith("Limit for rows to GROUP BY exceeded: has 11 rows, maximum: 10")
    assert len(ag) == 11


def test_break_mode(ch):
    ctx = ch.Context(0)
    ag = ch.Aggregator(np.uint64, [(ch.AGG_COUNT, None)], ctx=ctx, max_rows_to_group_by=10, group_by_overflow_mode="break")
    assert ag.execute_on_block(ctx.upload(np.arange(10, dtype=np.uint64)), [None]) is True
    assert ag.execute_on_block(ctx.upload(np.arange(12, dtype=np.uint64)), [None]) is False
    assert ag.execute_on_block(ctx.upload(np.arange(12, dtype=np.uint64)), [None]) is False   # not latched: the caller went on
    keys, res = ag.convert_to_block()
    got = dict(zip(keys.tolist(), res[0].tolist()))
    assert got == {k: (3 if k < 10 else 2) for k in range(12)}


def test_overflow_row_contents_and_float_window(ch):
    ctx = ch.Context(0)
    aggs = [(ch.AGG_COUNT, None), (ch.AGG_SUM, np.int64), (ch.AGG_AVG, np.float64), (ch.AGG_SUM, np.float64), (ch.AGG_MIN, np.int32),
            (ch.AGG_MAX, np.int32), (ch.AGG_ANY, np.int32)]
    ag = ch.Aggregator(np.uint64, aggs, ctx=ctx, max_rows_to_group_by=3, group_by_overflow_mode="any", overflow_row=True)
    assert ag.overflow_row() is None                          # none before the first block

    def blk(keys, ints, floats):
        k = ctx.upload(np.array(keys, dtype=np.uint64))
        i = ctx.upload(np.array(ints, dtype=np.int64))
        f = ctx.upload(np.array(floats, dtype=np.float64))
        i32 = ctx.upload(np.array(ints, dtype=np.int32))
        return ag.execute_on_block(k, [None, i, f, f, i32, i32, i32])

    blk([1, 2, 3, 4], [1, 2, 3, 4], [0.5, 0.25, 1.0, 2.0])
    o = [c.numpy()[0] for c in ag.overflow_row()]
    assert o[0] == 0 and o[1] == 0 and np.isnan(o[2]) and o[3] == 0.0 and o[4:] == [0, 0, 0]   # defaults when nothing missed
    blk([9, 1, 8], [-5, 100, 7], [0.125, 1.0, 0.75])
    blk([7, 2], [11, 1], [2.0**40, 3.0])                     # widens the fixed-point window while the overflow row holds values
    o = [c.numpy()[0] for c in ag.overflow_row()]
    assert o[0] == 3 and o[1] == 13 and o[2] == (0.125 + 0.75 + 2.0**40) / 3 and o[3] == 0.125 + 0.75 + 2.0**40
    assert (o[4], o[5], o[6]) == (-5, 11, -5)
    assert len(ag) == 4


def _limited_pair(ch, ctx, mode, ovf_on):
    aggs = [(ch.AGG_COUNT, None), (ch.AGG_SUM, np.int64)]
    x = ch.Aggregator(np.uint64, aggs, ctx=ctx, max_rows_to_group_by=5, group_by_overflow_mode=mode, overflow_row=ovf_on)
    y = ch.Aggregator(np.uint64, aggs, ctx=ctx)
    from clickhouse_amd import _capi as K
    try:   # 6 groups > 5: THROW fails here, with the block added
        x.execute_on_block(ctx.upload(np.arange(1, 7, dtype=np.uint64)), [None, ctx.upload(np.arange(1, 7, dtype=np.int64))])
    except K.ChgpuError as e:
        assert mode == "throw" and e.code == K.ERR_TOO_MANY_ROWS
    y.execute_on_block(ctx.upload(np.arange(4, 10, dtype=np.uint64)), [None, ctx.upload(np.full(6, 10, dtype=np.int64))])
    return x, y


@pytest.mark.parametrize("ovf_on", [True, False])
@pytest.mark.parametrize("mode", ["throw", "break", "any"])
def test_merge_under_limits(ch, mode, ovf_on):
    from clickhouse_amd import _capi as K
    ctx = ch.Context(0)
    x, y = _limited_pair(ch, ctx, mode, ovf_on)
    if mode == "throw":
        with pytest.raises(K.ChgpuError) as e:
            x.merge(y)
        assert e.value.code == K.ERR_TOO_MANY_ROWS
        return
    keep = x.merge(y)
    keys, res = x.convert_to_block()
    got = dict(zip(keys.tolist(), zip(res[0].tolist(), res[1].tolist())))
    base = {k: (1, k) for k in range(1, 7)}
    if mode == "break":
        assert keep is False and got == base
        assert (x.overflow_row() is None) == (not ovf_on)
    else:
        assert keep is True
        assert got == {k: (v[0] + (1 if k >= 4 else 0), v[1] + (10 if k >= 4 else 0)) for k, v in base.items()}
        o = x.overflow_row()
        if ovf_on:
            assert [c.numpy()[0] for c in o] == [3, 30]           # keys 7, 8, 9 of the source
        else:
            assert o is None


def test_merge_states_with_an_overflows_block(ch):
    ctx = ch.Context(0)
    aggs = [(ch.AGG_COUNT, None), (ch.AGG_SUM, np.int64)]
    x = ch.Aggregator(np.uint64, aggs, ctx=ctx, max_rows_to_group_by=2, group_by_overflow_mode="any", overflow_row=True)
    x.execute_on_block(ctx.upload(np.array([1, 2, 3], dtype=np.uint64)), [None, ctx.upload(np.array([1, 2, 3], dtype=np.int64))])
    assert x.no_more_keys
    sk = ctx.upload(np.array([3, 4], dtype=np.uint64))
    x.merge_states(sk, [ctx.upload(np.array([2, 5], dtype=np.uint64)), ctx.upload(np.array([20, 50], dtype=np.uint64))], 2)
    x.merge_states(None, [ctx.upload(np.array([7], dtype=np.uint64)), ctx.upload(np.array([70], dtype=np.uint64))], 1, is_overflows=True)
    keys, res = x.convert_to_block()
    assert dict(zip(keys.tolist(), zip(res[0].tolist(), res[1].tolist()))) == {1: (1, 1), 2: (1, 2), 3: (3, 23)}
    assert [c.numpy()[0] for c in x.overflow_row()] == [12, 120]
    blocks = x.convert_to_blocks()
    assert blocks[0].is_overflows and blocks[0].rows == 1 and not blocks[1].is_overflows


def test_overflow_rows_round_trip_through_the_merging_transform(ch):
    from clickhouse_amd.merging import MergingAggregatedMemoryEfficientTransform
    ctx = ch.Context(0)
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None), (ch.AGG_AVG, np.int64)]
    parts = []
    for s in range(2):
        a = ch.Aggregator(np.uint64, aggs, ctx=ctx, max_rows_to_group_by=2, group_by_overflow_mode="any", overflow_row=True)
        v = ctx.upload(np.array([1, 2, 3, 4, 5], dtype=np.int64) * (s + 1))
        a.execute_on_block(ctx.upload(np.array([1, 2, 3, 9, 10], dtype=np.uint64)), [v, None, v])
        a.execute_on_block(ctx.upload(np.array([1, 2, 11, 12, 13], dtype=np.uint64)), [v, None, v])
        parts.append(a)
    t = MergingAggregatedMemoryEfficientTransform(np.uint64, aggs, num_inputs=2, final=True, ctx=ctx)
    for i, a in enumerate(parts):
        words = a.overflow_row(final=False)
        t.add_chunk(i, ctx.upload(np.zeros(1, dtype=np.uint64)), words, is_overflows=True)
        t.finish_input(i)
    out = t.pull()
    ovf = [b for b in (out if isinstance(out, list) else [out]) if b is not None and b.is_overflows]
    assert len(ovf) == 1
    cols = [np.asarray(c.numpy() if hasattr(c, "numpy") else c) for c in ovf[0].columns]
    # each part: block 2 (find-only) misses keys 11, 12, 13 -> values 3 + 4 + 5, scaled by s + 1
    assert int(cols[0][0]) == 12 + 24 and int(cols[1][0]) == 6 and float(cols[2][0]) == 36 / 6


@pytest.mark.parametrize("limited", [True, False])
def test_zero_aggregate_functions(ch, limited):
    ctx = ch.Context(0)
    kw = dict(max_rows_to_group_by=3, group_by_overflow_mode="any", overflow_row=True) if limited else {}
    ag = ch.Aggregator(np.uint32, [], ctx=ctx, **kw)
    ag.execute_on_block(ctx.upload(np.array([5, 6, 7, 8, 5], dtype=np.uint32)), [])
    assert ag.no_more_keys == limited
    ag.execute_on_block(ctx.upload(np.array([1, 2, 3], dtype=np.uint32)), [])
    assert len(ag) == (4 if limited else 7)


def test_keys128_dictionary_stops_growing(ch):
    from clickhouse_amd.keysfixed import KeysFixedAggregator
    ctx = ch.Context(0)
    ag = KeysFixedAggregator([np.uint64, np.uint64], [(ch.AGG_COUNT, None)], ctx=ctx, max_rows_to_group_by=10, group_by_overflow_mode="any",
                             overflow_row=True)
    a = np.arange(20, dtype=np.uint64)
    ag.execute_on_block([a, a * 3], [None])
    assert ag.no_more_keys
    size = len(ag.dict)
    b = np.arange(10, 40, dtype=np.uint64)
    ag.execute_on_block([b, b * 3], [None])
    assert len(ag) == 20 and len(ag.dict) == size
    assert [c.numpy()[0] for c in ag.overflow_row()] == [20]


def test_without_key_limits_never_trigger(ch):
    ctx = ch.Context(0)
    ag = ch.Aggregator(None, [(ch.AGG_SUM, np.int64)], ctx=ctx, max_rows_to_group_by=1, group_by_overflow_mode="throw", overflow_row=True)
    for _ in range(3):
        assert ag.execute_on_block(None, [ctx.upload(np.ones(5, dtype=np.int64))]) is True
    assert ag.overflow_row() is None
    _, res = ag.convert_to_block()
    assert res[0].tolist() == [15]


def test_default_behaviour_is_add_block(ch):
    # the limited entry point with a limit that is never reached answers what chgpu_agg_add_block answers
    ctx = ch.Context(0)
    rng = _rng(3)
    k = rng.integers(0, 5000, size=300_000, dtype=np.uint64)
    v = rng.integers(-100, 100, size=300_000, dtype=np.int64)
    x = ch.Aggregator(np.uint64, [(ch.AGG_COUNT, None), (ch.AGG_SUM, np.int64)], ctx=ctx, max_rows_to_group_by=10**12,
                      group_by_overflow_mode="throw")
    assert x.limited
    y = ch.Aggregator(np.uint64, [(ch.AGG_COUNT, None), (ch.AGG_SUM, np.int64)], ctx=ctx)
    assert x.execute_on_block(ctx.upload(k), [None, ctx.upload(v)]) is True
    kc, vc = ctx.upload(k), ctx.upload(v)
    from clickhouse_amd import _capi as K
    import ctypes as C
    ptrs = (C.c_void_p * 2)(None, vc._h)
    K.check(K.lib().chgpu_agg_add_block(y._h, kc._h, ptrs, 0, len(k)))
    (kx, rx), (ky, ry) = x.convert_to_block(), y.convert_to_block()
    ox, oy = np.argsort(kx), np.argsort(ky)
    assert np.array_equal(kx[ox], ky[oy]) and all(np.array_equal(a[ox], b[oy]) for a, b in zip(rx, ry))
    assert x.overflow_row() is None


def test_set_limits_checks(ch):
    from clickhouse_amd import _capi as K
    ctx = ch.Context(0)
    ag = ch.Aggregator(np.uint64, [(ch.AGG_COUNT, None)], ctx=ctx)
    assert K.lib().chgpu_agg_set_limits(ag._h, 5, 3, 0) == K.ERR_BAD_ARGUMENTS
    ag.execute_on_block(ctx.upload(np.arange(3, dtype=np.uint64)), [None])
    assert K.lib().chgpu_agg_set_limits(ag._h, 5, K.OVERFLOW_ANY, 0) == K.ERR_BAD_ARGUMENTS


def test_overflows_blocks_widen_the_fixed_point_window_before_any_table(ch):
    # a fresh aggregator that first receives is_overflows blocks has an overflow row and no table: a second block with a larger exponent
    # widens the Float64 sums' window, which must move the overflow row's pair too
    ctx = ch.Context(0)
    x = ch.Aggregator(np.uint64, [(ch.AGG_SUM, np.float64), (ch.AGG_COUNT, None)], ctx=ctx, max_rows_to_group_by=5, group_by_overflow_mode="any",
                      overflow_row=True)
    vals = [0.375, 2.0**45 + 0.5, 2.0**70]
    for i, f in enumerate(vals):
        x.merge_states(None, [ctx.upload(np.array([f], dtype=np.float64)), ctx.upload(np.array([i + 1], dtype=np.uint64))], 1, is_overflows=True)
    assert len(x) == 0
    o = [c.numpy()[0] for c in x.overflow_row()]
    import math
    assert o[0] == math.fsum(vals) and o[1] == 6


def test_several_missed_any_states_merge_into_one_of_them(ch):
    ctx = ch.Context(0)
    aggs = [(ch.AGG_ANY, np.int64), (ch.AGG_COUNT, None)]
    x = ch.Aggregator(np.uint64, aggs, ctx=ctx, max_rows_to_group_by=2, group_by_overflow_mode="any", overflow_row=True)
    x.execute_on_block(ctx.upload(np.array([1, 2, 3], dtype=np.uint64)), [ctx.upload(np.array([10, 20, 30], dtype=np.int64)), None])
    y = ch.Aggregator(np.uint64, aggs, ctx=ctx)
    y.execute_on_block(ctx.upload(np.array([3, 7, 8, 9], dtype=np.uint64)), [ctx.upload(np.array([31, 70, 80, 90], dtype=np.int64)), None])
    assert x.merge(y) is True and x.merge_no_more_keys
    keys, res = x.convert_to_block()
    assert dict(zip(keys.tolist(), res[1].tolist())) == {1: 1, 2: 1, 3: 2}
    o = [c.numpy()[0] for c in x.overflow_row()]
    assert o[0] in (70, 80, 90) and o[1] == 3


def test_cpp_shim_limits_driver(tmp_path):
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(repo, "clickhouse_amd")
    if not os.path.exists(os.path.join(lib, "libchgpu.so")):
        import __graft_entry__ as g
        g.build()
    exe = str(tmp_path / "group_by_limits_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(repo, "tests", "group_by_limits_driver.cpp"), "-L" + lib, "-lchgpu", "-lpthread",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "group_by_limits_driver OK" in r.stdout
