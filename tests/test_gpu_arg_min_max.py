"""argMin(arg, val) / argMax(arg, val) states on the device (CHGPU_AGG_ARG_MIN / _MAX), bit-exact against the row-order restatement
in tests/arg_min_max_ref.py: the first row, over all blocks, that holds the group's extremum wins, whatever order the hardware serves
the rows in.  `arg` is compared as bytes.  No NaN in `val` except in the one test of the documented convention."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arg_min_max_ref as R  # noqa: E402
import keycraft as kc  # noqa: E402

pytestmark = pytest.mark.gpu

TYPES = ["int64", "uint32", "uint64", "float64", "uint8", "int32", "uint16", "int16", "int8", "float32"]


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    return ch.Context(0)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _b(x, dtype):
    return np.asarray(x, dtype=dtype).tobytes()


def _by_key(keys, col):
    """{key: the bytes of the group's value}"""
    return {int(k): col[i:i + 1].tobytes() for i, k in enumerate(keys.tolist())}


def _check(ag, refs):
    """refs: {result column index: Ref}"""
    keys, res = ag.convert_to_block()
    for j, ref in refs.items():
        assert res[j].dtype == ref.arg_dtype
        assert _by_key(keys, res[j]) == ref.result_bytes(), f"aggregate {j}"


def _vals(rng, dtype, n, spread=6):
    """a val column with many ties: signed types go negative, floats carry both infinities and both zeros"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        pool = np.array([-np.inf, -2.5, -0.0, 0.0, 1.25, 3.0, np.inf], dtype=dt)
        return pool[rng.integers(0, len(pool), size=n)]
    if dt.kind == "i":
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
        pool = np.array([lo, -3, -1, 0, 2, hi - 1, hi], dtype=dt)
        return pool[rng.integers(0, len(pool), size=n)]
    hi = np.iinfo(dt).max
    pool = np.array([0, 1, 2, hi // 2, hi - 1, hi], dtype=dt)
    return pool[rng.integers(0, len(pool), size=n)]


def _args(rng, dtype, n):
    """an arg column whose rows are (nearly) all different, so the winner's row is recognisable; floats carry a -0.0, Float64 raw NaN
    payloads too (Float32 travels through an exact widening, like any(): no signalling payloads there)"""
    dt = np.dtype(dtype)
    if dt == np.float64:
        a = rng.integers(0, 1 << 64, size=n, dtype=np.uint64).view(np.float64).copy()
        a[::97] = -0.0
        a[1::97] = np.array([0x7FF8_0000_0000_0ABC], dtype=np.uint64).view(np.float64)[0]
        return a
    if dt == np.float32:
        a = (rng.random(n) * 2e6 - 1e6).astype(np.float32)
        a[::97] = -0.0
        return a
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64).astype(dt) if dt.kind == "u" else rng.integers(-(1 << 63), 1 << 63, size=n, dtype=np.int64).astype(dt)


# ---- ties and lanes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [None, 99_999, 63, 64, 65, 255, 256])
def test_one_group_of_equal_val_the_first_row_wins(ch, ctx, at):
    n = 100_000
    keys = np.full(n, 7, dtype=np.uint64)
    arg = np.arange(n, dtype=np.int64)
    val = np.full(n, 5, dtype=np.int64)
    if at is not None:
        val[at] = 6  # the single maximum; argMin then ties over every other row
    ag = ch.Aggregator(np.uint64, [(ch.AGG_ARG_MAX, (np.int64, np.int64)), (ch.AGG_ARG_MIN, (np.int64, np.int64))], ctx=ctx)
    ag.execute_on_block(keys, [(arg, val), (arg, val)])
    gk, (mx, mn) = ag.convert_to_block()
    assert gk.tolist() == [7]
    assert int(mx[0]) == R.group_reference(keys, arg, val, False)[7] == (0 if at is None else at)
    assert int(mn[0]) == R.group_reference(keys, arg, val, True)[7] == 0


# ---- a stale claim ----------------------------------------------------------------------------------------------------------------
def test_a_raised_extremum_drops_the_stale_claim(ch, ctx):
    rng = _rng(11)
    G = 1000
    k1 = rng.permutation(np.repeat(np.arange(G, dtype=np.uint32), 3))
    v1 = rng.integers(0, 4, size=len(k1)).astype(np.int32)
    # block 2: half the groups get a new extremum (both directions), held by two of its rows -- the earlier must win; the other half
    # only sees values inside the old range
    raised = np.arange(0, G, 2, dtype=np.uint32)
    k2 = np.concatenate([raised, np.arange(1, G, 2, dtype=np.uint32), raised, raised])
    v2 = np.concatenate([np.full(len(raised), 9), rng.integers(1, 3, size=G // 2), np.full(len(raised), 9), np.full(len(raised), -9)]).astype(np.int32)
    p = rng.permutation(len(k2))
    k2, v2 = k2[p], v2[p]
    # block 3 only equals the extrema: nothing changes
    k3 = rng.permutation(np.repeat(raised, 2))
    v3 = np.where(rng.integers(0, 2, size=len(k3)) == 0, 9, -9).astype(np.int32)
    aggs = [(ch.AGG_ARG_MAX, (np.uint64, np.int32)), (ch.AGG_ARG_MIN, (np.uint64, np.int32))]
    ag = ch.Aggregator(np.uint32, aggs, ctx=ctx)
    rmax, rmin = R.Ref(False, np.uint64), R.Ref(True, np.uint64)
    base = 0
    snapshots = []
    for k, v in ((k1, v1), (k2, v2), (k3, v3)):
        a = np.arange(base, base + len(k), dtype=np.uint64)  # arg = the row's ordinal over all blocks
        base += len(k)
        ag.execute_on_block(k, [(a, v), (a, v)])
        rmax.add_block(k, a, v)
        rmin.add_block(k, a, v)
        snapshots.append(rmax.result_bytes())
    assert snapshots[1] != snapshots[0] and snapshots[2] == snapshots[1]
    _check(ag, {0: rmax, 1: rmin})


# ---- row ranges -------------------------------------------------------------------------------------------------------------------
def test_row_ranges_number_rows_by_ordinal_not_by_index(ch, ctx):
    rng = _rng(12)
    n = 30_000
    aggs = [(ch.AGG_ARG_MAX, (np.int64, np.int16)), (ch.AGG_ARG_MIN, (np.int64, np.int16))]
    ag = ch.Aggregator(np.uint16, aggs, ctx=ctx)
    rmax, rmin = R.Ref(False, np.int64), R.Ref(True, np.int64)
    # the second block's range starts at a LOWER index than the first block's: an index is no ordinal
    for seed, (lo, hi) in enumerate(((20_000, n - 500), (1_000, 9_999))):
        keys = rng.integers(0, 200, size=n).astype(np.uint16)
        val = _vals(rng, np.int16, n)
        arg = _args(rng, np.int64, n)
        ag.execute_on_block(keys, [(arg, val), (arg, val)], row_begin=lo, row_end=hi)
        rmax.add_block(keys, arg, val, row_begin=lo, row_end=hi)
        rmin.add_block(keys, arg, val, row_begin=lo, row_end=hi)
    _check(ag, {0: rmax, 1: rmin})


# ---- the type matrix --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("val_t", TYPES)
@pytest.mark.parametrize("arg_t", TYPES)
def test_type_matrix(ch, ctx, arg_t, val_t):
    rng = _rng(1000 + 16 * TYPES.index(arg_t) + TYPES.index(val_t))
    at, vt = np.dtype(arg_t), np.dtype(val_t)
    aggs = [(ch.AGG_ARG_MAX, (at, vt)), (ch.AGG_COUNT, None), (ch.AGG_ARG_MIN, (at, vt)), (ch.AGG_MAX, vt)]
    ag = ch.Aggregator(np.uint32, aggs, ctx=ctx)
    rmax, rmin = R.Ref(False, at), R.Ref(True, at)
    counts, maxima = {}, {}
    for _ in range(2):
        n = 2003
        keys = rng.integers(0, 300, size=n).astype(np.uint32)
        val, arg = _vals(rng, vt, n), _args(rng, at, n)
        ag.execute_on_block(keys, [(arg, val), None, (arg, val), val])
        rmax.add_block(keys, arg, val)
        rmin.add_block(keys, arg, val)
        for k, v in zip(keys.tolist(), val.tolist()):
            counts[k] = counts.get(k, 0) + 1
            maxima[k] = max(maxima.get(k, v), v)
    _check(ag, {0: rmax, 2: rmin})
    gk, res = ag.convert_to_block()
    assert dict(zip(gk.tolist(), res[1].tolist())) == counts
    assert dict(zip(gk.tolist(), res[3].tolist())) == maxima  # (numeric: max() keeps its own order key, +0.0 above -0.0)


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
def test_uint8_keys_and_the_zero_key(ch, ctx):
    rng = _rng(13)
    aggs = [(ch.AGG_ARG_MAX, (np.float64, np.float32)), (ch.AGG_ARG_MIN, (np.float64, np.float32))]
    ag = ch.Aggregator(np.uint8, aggs, ctx=ctx)
    rmax, rmin = R.Ref(False, np.float64), R.Ref(True, np.float64)
    for _ in range(3):
        n = 5000
        keys = rng.integers(0, 256, size=n).astype(np.uint8)
        keys[:7] = 0
        val, arg = _vals(rng, np.float32, n), _args(rng, np.float64, n)
        ag.execute_on_block(keys, [(arg, val), (arg, val)])
        rmax.add_block(keys, arg, val)
        rmin.add_block(keys, arg, val)
    assert 0 in rmax.states and len(ag) == len(rmax.states)
    _check(ag, {0: rmax, 1: rmin})


def test_keys_that_share_one_home_cell_walk_the_probe_chain(ch, ctx):
    # the table has 2^22 cells until it grows (AGG_MIN_CAPACITY) and places a key at intHash64(key) & (cells - 1): 48 keys with one home
    rng = _rng(14)
    lg = 22
    home = 0x2ABCD
    crafted = kc.int_hash64_inv((np.arange(1, 49, dtype=np.uint64) << np.uint64(lg)) | np.uint64(home))
    assert np.all((kc.int_hash64(crafted) & np.uint64((1 << lg) - 1)) == home) and len(set(crafted.tolist())) == 48 and 0 not in crafted
    aggs = [(ch.AGG_ARG_MAX, (np.uint32, np.uint8)), (ch.AGG_ARG_MIN, (np.uint32, np.uint8))]
    ag = ch.Aggregator(np.uint64, aggs, ctx=ctx)
    rmax, rmin = R.Ref(False, np.uint32), R.Ref(True, np.uint32)
    for _ in range(2):
        n = 6000
        keys = crafted[rng.integers(0, 48, size=n)]
        val, arg = _vals(rng, np.uint8, n), _args(rng, np.uint32, n)
        ag.execute_on_block(keys, [(arg, val), (arg, val)])
        rmax.add_block(keys, arg, val)
        rmin.add_block(keys, arg, val)
    _check(ag, {0: rmax, 1: rmin})


def test_nullable_and_wide_key_aggregators_pass_the_pair_through(ch, ctx):
    rng = _rng(25)
    n = 5000
    aggs = [(ch.AGG_ARG_MAX, (np.int64, np.int16)), (ch.AGG_COUNT, None), (ch.AGG_ARG_MIN, (np.int64, np.int16))]
    keys = rng.integers(0, 100, size=n).astype(np.uint32)
    nm = (rng.random(n) < 0.1).astype(np.uint8)
    val, arg = _vals(rng, np.int16, n), _args(rng, np.int64, n)
    # Nullable key: the NULL rows go to an aggregation without key, whatever their nested value
    N = ch.NullableKeyAggregator(np.uint32, aggs, ctx=ctx)
    N.execute_on_block(keys, nm, [(arg, val), None, (arg, val)])
    gk, nulls, res = N.convert_to_block()
    assert nulls.tolist() == [0] * (len(gk) - 1) + [1]
    for j, is_min in ((0, False), (2, True)):
        keyed, null = R.Ref(is_min, np.int64), R.Ref(is_min, np.int64)
        keyed.add_block(keys, arg, val, mask=1 - nm)
        null.add_block(None, arg, val, mask=nm)
        assert _by_key(gk[:-1], res[j][:-1]) == keyed.result_bytes()
        assert res[j][-1:].tobytes() == null.result_bytes()[None]
    # two UInt64 key columns (keys128: the wide-key dictionary in front of the aggregator), a row range
    k2 = rng.integers(0, 3, size=n).astype(np.uint64)
    W = ch.KeysFixedAggregator([np.uint64, np.uint64], aggs, ctx=ctx)
    W.execute_on_block([keys.astype(np.uint64), k2], [(arg, val), None, (arg, val)], row_begin=100, row_end=n - 100)
    (w1, w2), wres = W.convert_to_block()
    packed = keys.astype(np.uint64) * np.uint64(4) + k2
    for j, is_min in ((0, False), (2, True)):
        ref = R.Ref(is_min, np.int64)
        ref.add_block(packed, arg, val, row_begin=100, row_end=n - 100)
        assert _by_key(w1 * np.uint64(4) + w2, wres[j]) == ref.result_bytes()


# ---- table growth -------------------------------------------------------------------------------------------------------------------
def test_states_survive_the_rehash_of_a_grown_table(ch, ctx):
    """the one large shape: more than 2 Mi groups (half of AGG_MIN_CAPACITY) are needed to reach the rehash at all"""
    rng = _rng(15)
    n, block = 4_500_000, 65_409
    keys = rng.integers(1, 3_200_000, size=n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    keys[:3] = 0
    val = rng.integers(-3, 4, size=n).astype(np.int8)      # ties within and across blocks, before and after the rehash
    arg = np.arange(n, dtype=np.uint32)                    # the winner's row itself
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    aggs = [(ch.AGG_ARG_MAX, (np.uint32, np.int8)), (ch.AGG_ARG_MIN, (np.uint32, np.int8)), (ch.AGG_COUNT, None)]
    ag = ch.Aggregator(np.uint64, aggs, ctx=ctx)
    kcol, acol, vcol, mcol = ctx.upload(keys), ctx.upload(arg), ctx.upload(val), ctx.upload(mask)
    for b in range(0, n, block):
        ag.execute_on_block(kcol, [(acol, vcol), (acol, vcol), None], row_begin=b, row_end=min(n, b + block), filter=mcol)
    gk, (mx, mn, cnt) = ag.convert_to_block()
    assert len(gk) > (1 << 21)
    order = np.argsort(gk)
    for got, is_min in ((mx, False), (mn, True)):
        wk, wr = R.group_reference_arrays(keys, arg, val, is_min, mask)
        assert np.array_equal(gk[order], wk)
        assert np.array_equal(got[order], arg[wr])
    assert int(cnt.sum()) == int(mask.sum())


# ---- merge and states ---------------------------------------------------------------------------------------------------------------
def _merge_blocks(rng):
    """A holds keys 0..299, B holds 200..499: over 200..299 B is strictly greater in a third, equal in a third, smaller in a third"""
    ka = rng.permutation(np.repeat(np.arange(0, 300, dtype=np.uint64), 4))
    va = rng.integers(10, 13, size=len(ka)).astype(np.int64)
    kb = rng.permutation(np.repeat(np.arange(200, 500, dtype=np.uint64), 4))
    vb = np.where(kb % 3 == 0, 20, np.where(kb % 3 == 1, 12, 5)).astype(np.int64)
    vb[kb >= 300] = rng.integers(-4, 4, size=int((kb >= 300).sum()))
    return (ka, va, _args(rng, np.int16, len(ka))), (kb, vb, _args(rng, np.int16, len(kb)))


AGGS_I16_I64 = lambda ch: [(ch.AGG_ARG_MAX, (np.int16, np.int64)), (ch.AGG_COUNT, None), (ch.AGG_ARG_MIN, (np.int16, np.int64))]  # noqa: E731


def _feed(ag, refs, k, a, v):
    ag.execute_on_block(k, [(a, v), None, (a, v)])
    for r in refs:
        r.add_block(k, a, v)


def test_merge_keeps_the_destination_on_equal_val(ch, ctx):
    rng = _rng(16)
    (ka, va, aa), (kb, vb, ab) = _merge_blocks(rng)
    A, B = ch.Aggregator(np.uint64, AGGS_I16_I64(ch), ctx=ctx), ch.Aggregator(np.uint64, AGGS_I16_I64(ch), ctx=ctx)
    ra, rb = [R.Ref(False, np.int16), R.Ref(True, np.int16)], [R.Ref(False, np.int16), R.Ref(True, np.int16)]
    _feed(A, ra, ka, aa, va)
    _feed(B, rb, kb, ab, vb)
    A.merge(B)
    for x, y in zip(ra, rb):
        x.merge(y)
    _check(A, {0: ra[0], 2: ra[1]})
    # a further block whose rows EQUAL the merged-in extrema (and the ones A kept): every one of them must lose
    k3 = np.arange(0, 500, dtype=np.uint64)
    for is_min, ref in ((False, ra[0]), (True, ra[1])):
        v3 = np.array([R.M64 - ref.states[int(k)].key if is_min else ref.states[int(k)].key for k in k3], dtype=np.uint64)
        v3 = (v3 ^ np.uint64(R.SIGN)).view(np.int64)  # the order key of a signed value, undone
        before = ref.result_bytes()
        _feed(A, ra, k3, _args(rng, np.int16, len(k3)), v3)
        assert ref.result_bytes() == before
    _check(A, {0: ra[0], 2: ra[1]})


def test_state_columns_are_three_words_and_merge_back(ch, ctx):
    rng = _rng(17)
    (ka, va, aa), (kb, vb, ab) = _merge_blocks(rng)
    A, B = ch.Aggregator(np.uint64, AGGS_I16_I64(ch), ctx=ctx), ch.Aggregator(np.uint64, AGGS_I16_I64(ch), ctx=ctx)
    ra, rb = [R.Ref(False, np.int16), R.Ref(True, np.int16)], [R.Ref(False, np.int16), R.Ref(True, np.int16)]
    _feed(A, ra, ka, aa, va)
    _feed(B, rb, kb, ab, vb)
    keys, words, rows = B.export_state_columns()
    assert len(words) == B.n_words == 3 + 1 + 3 and rows == 300
    k = keys.numpy()
    w = [c.numpy() for c in words]
    for i, key in enumerate(k.tolist()):
        for base, ref in ((0, rb[0]), (4, rb[1])):
            st = ref.states[key]
            assert int(w[base][i]) == st.key and int(w[base + 1][i]) != 0
            assert w[base + 2][i:i + 1].astype(np.uint64).astype(np.uint16).tobytes() == _b(st.arg, np.int16)
    # into an empty aggregation
    E = ch.Aggregator(np.uint64, AGGS_I16_I64(ch), ctx=ctx)
    E.merge_states(keys, words, rows)
    _check(E, {0: rb[0], 2: rb[1]})
    # into one that holds rows; the two-level export of B carries the same states
    k2, words2, rows2, counts = B.export_state_columns_two_level()
    assert rows2 == 300 and sum(counts) == 300 and len(words2) == 7
    A.merge_states(k2, words2, rows2)
    for x, y in zip(ra, rb):
        x.merge(y)
    _check(A, {0: ra[0], 2: ra[1]})
    # `has` reads as a flag: any non-zero value is "has a value, older than every row to come"; 0 loses every merge
    F = ch.Aggregator(np.uint64, AGGS_I16_I64(ch), ctx=ctx)
    fk = np.array([1, 2], dtype=np.uint64)
    cols = [np.array([50, 50], dtype=np.uint64), np.array([1, 0], dtype=np.uint64), np.array([111, 222], dtype=np.uint64), np.array([1, 1], dtype=np.uint64),
            np.array([50, 50], dtype=np.uint64), np.array([12345, 0], dtype=np.uint64), np.array([333, 444], dtype=np.uint64)]
    F.merge_states(ctx.upload(fk), [ctx.upload(c) for c in cols], 2)
    tie = np.array([50 ^ R.SIGN], dtype=np.uint64).view(np.int64)          # val whose argMax key is 50
    tie_min = np.array([(R.M64 - 50) ^ R.SIGN], dtype=np.uint64).view(np.int64)  # ... whose argMin key is 50
    F.execute_on_block(fk, [(np.array([7, 8], dtype=np.int16), np.repeat(tie, 2)), None, (np.array([7, 8], dtype=np.int16), np.repeat(tie_min, 2))])
    gk, res = F.convert_to_block()
    got = {int(key): (int(res[0][i]), int(res[2][i])) for i, key in enumerate(gk.tolist())}
    assert got == {1: (111, 333), 2: (8, 8)}


# ---- without key --------------------------------------------------------------------------------------------------------------------
def test_without_key(ch, ctx):
    rng = _rng(18)
    aggs = [(ch.AGG_ARG_MAX, (np.uint64, np.float64)), (ch.AGG_ARG_MIN, (np.uint64, np.float64)), (ch.AGG_COUNT, None)]
    W, W2 = ch.Aggregator(None, aggs, ctx=ctx), ch.Aggregator(None, aggs, ctx=ctx)
    refs, refs2 = [R.Ref(False, np.uint64), R.Ref(True, np.uint64)], [R.Ref(False, np.uint64), R.Ref(True, np.uint64)]
    n = 3 * 20_011
    val, arg = _vals(rng, np.float64, n), _args(rng, np.uint64, n)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    mask[:20_011] = 0  # the first block passes nothing: the state must wait for the second
    for b in range(0, n, 20_011):
        s = slice(b, b + 20_011)
        W.execute_on_block(None, [(arg[s], val[s]), (arg[s], val[s]), None], filter=mask[s])
        for r in refs:
            r.add_block(None, arg[s], val[s], mask=mask[s])
        if b == 0:
            _, res = W.convert_to_block()
            assert [int(x[0]) for x in res] == [0, 0, 0]  # no value yet: arg's default
    v2, a2 = _vals(rng, np.float64, 999), _args(rng, np.uint64, 999)
    W2.execute_on_block(None, [(a2, v2), (a2, v2), None])
    for r in refs2:
        r.add_block(None, a2, v2)

    def same(ag, rr):
        _, res = ag.convert_to_block()
        assert [res[0].tobytes(), res[1].tobytes()] == [r.result_bytes()[None] for r in rr]
    same(W, refs)
    same(W2, refs2)
    # export / import into an empty aggregation, then merge: equal val keeps the destination
    _, words, rows = W2.export_state_columns()
    assert len(words) == 7 and rows == 1
    E = ch.Aggregator(None, aggs, ctx=ctx)
    E.merge_states(None, words, 1)
    same(E, refs2)
    W.merge(W2)
    for x, y in zip(refs, refs2):
        x.merge(y)
    same(W, refs)
    # a row that equals the merged extremum loses
    top = np.array([np.inf, -np.inf])
    W.execute_on_block(None, [(np.array([1, 2], dtype=np.uint64), top), (np.array([1, 2], dtype=np.uint64), top), None])
    same(W, refs)
    # empty input
    Z = ch.Aggregator(None, aggs, ctx=ctx)
    _, res = Z.convert_to_block()
    assert [int(x[0]) for x in res] == [0, 0, 0]
    Z.merge(W2)
    same(Z, refs2)


# ---- limits -------------------------------------------------------------------------------------------------------------------------
def _limit_blocks(rng):
    A = np.arange(1, 201, dtype=np.uint32)
    B = np.arange(1000, 1300, dtype=np.uint32)
    k1 = rng.permutation(np.repeat(A, 3))
    k2 = rng.permutation(np.concatenate([np.repeat(A, 2), np.repeat(B, 40)]))  # 12 000 missed rows fold into ONE overflow state
    return A, (k1, _vals(rng, np.int32, len(k1)), _args(rng, np.int64, len(k1))), (k2, _vals(rng, np.int32, len(k2)), _args(rng, np.int64, len(k2)))


@pytest.mark.parametrize("ovf_on", [True, False])
def test_overflow_mode_any_folds_missed_rows_with_the_same_tie_rule(ch, ctx, ovf_on):
    rng = _rng(19 + ovf_on)
    A, (k1, v1, a1), (k2, v2, a2) = _limit_blocks(rng)
    aggs = [(ch.AGG_ARG_MAX, (np.int64, np.int32)), (ch.AGG_ARG_MIN, (np.int64, np.int32))]
    ag = ch.Aggregator(np.uint32, aggs, ctx=ctx, max_rows_to_group_by=len(A) - 1, group_by_overflow_mode="any", overflow_row=ovf_on)
    refs = [R.Ref(False, np.int64), R.Ref(True, np.int64)]
    ovf = [R.State(), R.State()]
    assert ag.execute_on_block(k1, [(a1, v1), (a1, v1)]) is True and ag.no_more_keys
    for r in refs:
        r.add_block(k1, a1, v1)
    for rep in range(2):  # the second find-only block only ties or loses against the overflow row of the first... or raises it
        kk, vv, aa = (k2, v2, a2) if rep == 0 else (k2[::-1].copy(), v2[::-1].copy(), _args(rng, np.int64, len(k2)))
        assert ag.execute_on_block(kk, [(aa, vv), (aa, vv)]) is True
        for r, o in zip(refs, ovf):
            r.add_block_find_only(kk, aa, vv, o if ovf_on else None)
    assert len(ag) == len(A)
    _check(ag, {0: refs[0], 1: refs[1]})
    final = ag.overflow_row(final=True)
    if not ovf_on:
        assert final is None
        return
    assert [c.numpy().tobytes() for c in final] == [_b(r.result_of(o), np.int64) for r, o in zip(refs, ovf)]
    words = [int(c.numpy().view(np.uint64)[0]) for c in ag.overflow_row(final=False)]
    assert len(words) == 6
    for base, o in ((0, ovf[0]), (3, ovf[1])):
        assert words[base] == o.key and words[base + 1] != 0 and words[base + 2] == int(np.asarray(o.arg).astype(np.int64).view(np.uint64))


def test_an_overflow_row_nobody_reached_has_no_value(ch, ctx):
    aggs = [(ch.AGG_ARG_MAX, (np.int64, np.int32))]
    ag = ch.Aggregator(np.uint32, aggs, ctx=ctx, max_rows_to_group_by=100, group_by_overflow_mode="any", overflow_row=True)
    ag.execute_on_block(np.arange(5, dtype=np.uint32), [(np.arange(5, dtype=np.int64) + 9, np.zeros(5, dtype=np.int32))])
    assert [int(c.numpy()[0]) for c in ag.overflow_row(final=True)] == [0]
    assert [int(c.numpy().view(np.uint64)[0]) for c in ag.overflow_row(final=False)][1] == 0


def test_merge_under_no_more_keys_folds_source_states_into_the_overflow_row(ch, ctx):
    rng = _rng(21)
    aggs = [(ch.AGG_ARG_MAX, (np.int64, np.int32)), (ch.AGG_ARG_MIN, (np.int64, np.int32))]
    D = ch.Aggregator(np.uint32, aggs, ctx=ctx, max_rows_to_group_by=50, group_by_overflow_mode="any", overflow_row=True)
    S = ch.Aggregator(np.uint32, aggs, ctx=ctx)
    kd = np.arange(1, 101, dtype=np.uint32)
    vd, ad = _vals(rng, np.int32, 100), _args(rng, np.int64, 100)
    ks = rng.permutation(np.arange(51, 3051, dtype=np.uint32))  # 50 keys D has, 2950 it lacks: those fall into the overflow row, with many ties
    vs, as_ = _vals(rng, np.int32, len(ks)), _args(rng, np.int64, len(ks))
    D.execute_on_block(kd, [(ad, vd), (ad, vd)])
    S.execute_on_block(ks, [(as_, vs), (as_, vs)])
    rd, rs = [R.Ref(False, np.int64), R.Ref(True, np.int64)], [R.Ref(False, np.int64), R.Ref(True, np.int64)]
    for r in rd:
        r.add_block(kd, ad, vd)
    # the source's states merge in the order of its table, which is the order it exports them in
    src_order, _ = S.convert_to_block()
    pos = {int(k): i for i, k in enumerate(ks.tolist())}
    idx = np.array([pos[int(k)] for k in src_order.tolist()])
    for r in rs:
        r.add_block(ks[idx], as_[idx], vs[idx])
    assert D.merge(S) is True and D.merge_no_more_keys
    ovf = [R.State(), R.State()]
    for x, y, o in zip(rd, rs, ovf):
        x.merge(y, find_only=True, overflow=o)
    assert len(D) == 100
    _check(D, {0: rd[0], 1: rd[1]})
    assert [c.numpy().tobytes() for c in D.overflow_row(final=True)] == [_b(r.result_of(o), np.int64) for r, o in zip(rd, ovf)]


@pytest.mark.parametrize("mode", ["throw", "break"])
def test_throw_and_break_behave_as_for_max(ch, ctx, mode):
    rng = _rng(22)
    keys = np.arange(300, dtype=np.uint32)
    val, arg = _vals(rng, np.int32, 300), _args(rng, np.int64, 300)
    outcomes = []
    for aggs, args in (([(ch.AGG_ARG_MAX, (np.int64, np.int32))], [(arg, val)]), ([(ch.AGG_MAX, np.int32)], [val])):
        ag = ch.Aggregator(np.uint32, aggs, ctx=ctx, max_rows_to_group_by=100, group_by_overflow_mode=mode)
        try:
            outcomes.append((ag.execute_on_block(keys, args), len(ag)))
        except ch._capi.ChgpuError as e:
            outcomes.append(("raised", e.code))
    assert outcomes[0] == outcomes[1] == (("raised", ch._capi.ERR_TOO_MANY_ROWS) if mode == "throw" else (False, 300))


# ---- NaN val: the documented convention only -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vt", [np.float32, np.float64])
def test_nan_val_takes_its_order_key_place_like_min_and_max(ch, ctx, vt):
    rng = _rng(23)
    n = 8000
    keys = rng.integers(0, 50, size=n).astype(np.uint32)
    val = (rng.integers(1, 9, size=n) * 0.5).astype(vt)  # no zeros
    val[rng.integers(0, n, size=400)] = np.nan
    val[rng.integers(0, n, size=400)] = -np.nan
    arg = np.arange(n, dtype=np.uint32)
    aggs = [(ch.AGG_ARG_MAX, (np.uint32, vt)), (ch.AGG_ARG_MIN, (np.uint32, vt)), (ch.AGG_MAX, vt), (ch.AGG_MIN, vt)]
    ag = ch.Aggregator(np.uint32, aggs, ctx=ctx)
    ag.execute_on_block(keys, [(arg, val), (arg, val), val, val])
    gk, (amx, amn, mx, mn) = ag.convert_to_block()
    assert val[amx].tobytes() == mx.tobytes() and val[amn].tobytes() == mn.tobytes()
    assert np.array_equal(keys[amx], gk) and np.array_equal(keys[amn], gk)
    rmax, rmin = R.Ref(False, np.uint32), R.Ref(True, np.uint32)
    rmax.add_block(keys, arg, val)
    rmin.add_block(keys, arg, val)
    _check(ag, {0: rmax, 1: rmin})


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_wire_serialisation_and_too_many_words_are_refused(ch, ctx):
    from clickhouse_amd.aggregator import serialize_states
    K = ch._capi
    w = ctx.upload(np.arange(4, dtype=np.uint64))
    for kind in (ch.AGG_ARG_MIN, ch.AGG_ARG_MAX):
        with pytest.raises(K.ChgpuError) as e:
            serialize_states(ctx, kind, w, w)
        assert e.value.code == K.ERR_NOT_IMPLEMENTED
    five = [(ch.AGG_ARG_MAX, (np.int64, np.int64))] * 5  # 15 state words: the last that fit
    ch.Aggregator(np.uint64, five, ctx=ctx).close()
    for aggs in (five + [(ch.AGG_ANY, np.int64)], [(ch.AGG_ARG_MIN, (np.int8, np.int8))] * 6):
        with pytest.raises(K.ChgpuError) as e:
            ch.Aggregator(np.uint64, aggs, ctx=ctx)
        assert e.value.code == K.ERR_NOT_IMPLEMENTED


# ---- the sites shared with any / max / count ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.int32, np.float64])
def test_any_max_count_still_match_the_oracle(ch, ctx, oracle_mod, dt):
    O = oracle_mod
    rng = _rng(24)
    n = 60_000
    keys = rng.integers(0, 5000, size=n, dtype=np.uint64)
    vals = (rng.random(n) * 200 - 100).astype(dt) if np.dtype(dt).kind == "f" else rng.integers(-100, 120, size=n).astype(dt)
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    aggs = [(ch.AGG_ANY, dt), (ch.AGG_MAX, dt), (ch.AGG_COUNT, None)]
    A, B, OA, OB = ch.Aggregator(np.uint64, aggs, ctx=ctx), ch.Aggregator(np.uint64, aggs, ctx=ctx), O.Aggregator(np.uint64, aggs), O.Aggregator(np.uint64, aggs)
    for g_, o_, lo, hi in ((A, OA, 0, n // 2), (B, OB, n // 2, n)):
        for b in range(lo, hi, 9973):
            e = min(hi, b + 9973)
            g_.execute_on_block(keys[b:e], [vals[b:e], vals[b:e], None], filter=mask[b:e])
            kept = mask[b:e] != 0
            o_.execute_on_block(keys[b:e][kept], [vals[b:e][kept], vals[b:e][kept], None])
    A.merge(B)
    OA.merge(OB)
    gk, gres = A.convert_to_block()
    ok, ores = OA.convert_to_block()
    i, q = np.argsort(gk), np.argsort(ok)
    assert np.array_equal(gk[i], ok[q])
    for g, o in zip(gres, ores):
        assert np.array_equal(g[i].view(np.uint8), np.asarray(o)[q].astype(g.dtype).view(np.uint8))
