"""uniqExact / count(DISTINCT) under GROUP BY on the device (clickhouse_amd/csrc/uniq_kernels.hip) against tests/uniq_exact_ref.py.

The device is compared to the reference as sets of (key bits, value bits) and as {key: count}, order-free.  Where a case claims a path
(the LDS stage, an overflow of the LDS set, a wrap, a growth) it also reads the `debug` option's `uniq plan=` line, so that it cannot pass
by another route; pairs with a chosen place in the tables come from tests/uniq_craft.py, which inverts the placement hash."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import uniq_craft as U  # noqa: E402
from uniq_exact_ref import UniqExactRef, bits, from_bits  # noqa: E402

pytestmark = pytest.mark.gpu

KEY_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
VALUE_DTYPES = KEY_DTYPES + [np.float32, np.float64]
TILE = U.UQ_TILE
LG = 20   # crafted global homes hold for every capacity up to 2^20 cells


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


def _plans(err):
    got = [ln[len("chgpu: "):] for ln in err.splitlines() if ln.startswith("chgpu: uniq plan=")]
    return [dict(kv.split("=", 1) for kv in ln.split() if "=" in kv) for ln in got]


def _add(u, capfd, keys, values, **kw):
    """add_block -> the call's plan line as a dict (ints; a->b fields as (a, b))"""
    capfd.readouterr()
    u.add_block(keys, values, **kw)
    plans = _plans(capfd.readouterr().err)
    assert len(plans) == 1, plans
    return _ints(plans[0])


def _ints(plan):
    out = {}
    for k, v in plan.items():
        out[k] = v if k == "plan" else tuple(int(x) for x in v.split("->")) if "->" in v else int(v)
    return out


def _device_pairs(u):
    k, v = u.export_pairs()
    kb = bits(k) if k is not None else np.zeros(len(v), dtype=np.uint64)
    return list(zip(kb.tolist(), bits(v).tolist()))


def _check(u, ref):
    """the device set equals the reference: as pairs (each exactly once), as a size and as {key: count}"""
    got = _device_pairs(u)
    assert len(got) == len(set(got)), "a pair was exported twice"
    assert set(got) == ref.pairs
    assert len(u) == len(ref)
    k, c = u.finalize()
    if ref.key_dtype is None:
        assert k is None and c.dtype == np.uint64 and c.tolist() == [len(ref)]
    else:
        assert k.dtype == ref.key_dtype and c.dtype == np.uint64
        d = dict(zip(bits(k).tolist(), c.tolist()))
        assert len(d) == len(k), "a key was finalised twice"
        assert d == ref.finalize()


def _patterns(rng, dtype, n):
    """n random bit patterns of dtype (floats: any bits, NaNs included)"""
    dtype = np.dtype(dtype)
    return from_bits(rng.integers(0, 1 << (8 * dtype.itemsize), size=n, dtype=np.uint64, endpoint=False) if dtype.itemsize < 8
                     else rng.integers(0, 2**64, size=n, dtype=np.uint64), dtype)


def _edges(dtype):
    """0, all-ones, the signed minimum; floats: +-0.0, +-inf and two NaN payloads"""
    dtype = np.dtype(dtype)
    w = 8 * dtype.itemsize
    words = [0, (1 << w) - 1, 1 << (w - 1)]
    if dtype.kind == "f":
        exp = {32: 0x7F800000, 64: 0x7FF0000000000000}[w]
        words += [exp, exp | (1 << (w - 1)), exp | 1, exp | 2, exp | (1 << (w - 2)) | 1]
    return from_bits(np.array(words, dtype=np.uint64), dtype)


def _matrix_block(rng, kd, vd, n=5000):
    """a few dozen keys, a few hundred values, most pairs repeated; the edge patterns planted, each special value twice"""
    vpool = np.concatenate([_patterns(rng, vd, 300), _edges(vd)])
    vi = None
    if kd is None:
        ki = np.zeros(n, dtype=np.int64)
        vi = rng.integers(0, 320, size=n) % len(vpool)
        keys = None
    else:
        kpool = np.concatenate([_patterns(rng, kd, 40), _edges(kd)])
        ki = rng.integers(0, len(kpool), size=n)
        vi = (ki * 7 + rng.integers(0, 8, size=n)) % len(vpool)
        # planted: every edge key with every edge value (the pair (0, 0), (all-ones, all-ones), the minima ...), twice each
        ne_k, ne_v = len(_edges(kd)), len(_edges(vd))
        pk = np.repeat(np.arange(len(kpool) - ne_k, len(kpool)), ne_v)
        pv = np.tile(np.arange(len(vpool) - ne_v, len(vpool)), ne_k)
        m = len(pk)
        ki[:m], vi[:m] = pk, pv
        ki[m:2 * m], vi[m:2 * m] = pk, pv
        keys = kpool[ki]
    if kd is None:
        ne_v = len(_edges(vd))
        vi[:ne_v] = np.arange(len(vpool) - ne_v, len(vpool))
        vi[ne_v:2 * ne_v] = vi[:ne_v]
    return keys, vpool[vi]


# ---- type matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vd", VALUE_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kd", KEY_DTYPES + [None], ids=lambda d: "nokey" if d is None else np.dtype(d).name)
def test_type_matrix(ch, ctx, capfd, kd, vd):
    rng = _rng(100 + len(np.dtype(vd).name) * 31 + (0 if kd is None else np.dtype(kd).num))
    keys, values = _matrix_block(rng, kd, vd)
    ref = UniqExactRef(kd, vd).add(keys, values)
    u = ch.UniqExact(kd, vd, ctx=ctx)
    try:
        plan = _add(u, capfd, keys, values)
        assert plan["n"] == len(values) and plan["tiles"] == -(-len(values) // TILE) and plan["rc"] == 0
        assert plan["lds"] + plan["sent"] == len(values) and plan["lds"] > len(values) // 2   # most rows die in LDS
        assert plan["slots"][1] - plan["holes"][1] == len(ref)
        _check(u, ref)
        if kd is not None:
            probe = np.concatenate([keys[:50], _edges(kd), _patterns(rng, kd, 20)])
            assert np.array_equal(u.counts_for_keys(probe), ref.counts_for_keys(probe))
    finally:
        u.close()


def test_float_keys_are_not_implemented(ch, ctx):
    for kd in (np.float32, np.float64):
        with pytest.raises(ch.ChgpuError) as e:
            ch.UniqExact(kd, np.int64, ctx=ctx)
        assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED


# ---- row selection ----------------------------------------------------------------------------------------------------------------
def _selection_block(rng, n=5000):
    keys = rng.integers(0, 30, size=n, dtype=np.uint32)
    values = rng.integers(-40, 40, size=n, dtype=np.int64)
    return keys, values


RANGES = [(rb, re) for rb in (0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1) for re in (rb + 1, rb + 256, TILE + 255, 2 * TILE, 2 * TILE + 1, 5000) if rb < re]


def test_row_ranges_either_side_of_a_tile_and_of_the_rows_per_lane_multiple(ch, ctx, capfd):
    keys, values = _selection_block(_rng(7))
    kcol, vcol = ctx.upload(keys), ctx.upload(values)
    for rb, re in RANGES:
        u = ch.UniqExact(np.uint32, np.int64, ctx=ctx)
        try:
            plan = _add(u, capfd, kcol, vcol, row_begin=rb, row_end=re)
            assert plan["n"] == re - rb and plan["tiles"] == -(-(re - rb) // TILE)
            _check(u, UniqExactRef(np.uint32, np.int64).add(keys, values, rb, re))
        finally:
            u.close()


def test_filter_bytes_0_1_2_255(ch, ctx, capfd):
    rng = _rng(8)
    keys, values = _selection_block(rng)
    filt = rng.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), size=len(keys))
    for kd in (np.uint32, None):
        u = ch.UniqExact(kd, np.int64, ctx=ctx)
        try:
            plan = _add(u, capfd, keys if kd else None, values, filter=filt, row_begin=3, row_end=4999)
            assert plan["lds"] + plan["sent"] == int(np.count_nonzero(filt[3:4999]))
            _check(u, UniqExactRef(kd, np.int64).add(keys if kd else None, values, 3, 4999, filter=filt))
        finally:
            u.close()


@pytest.mark.parametrize("kd", [np.uint32, None], ids=["keyed", "nokey"])
def test_nothing_enters(ch, ctx, capfd, kd):
    keys, values = _selection_block(_rng(9), 3000)
    ref = UniqExactRef(kd, np.int64)
    u = ch.UniqExact(kd, np.int64, ctx=ctx)
    try:
        k = keys if kd else None
        plan = _add(u, capfd, k, values, filter=np.zeros(3000, dtype=np.uint8))            # an all-zero filter
        assert (plan["lds"], plan["sent"], plan["slots"]) == (0, 0, (0, 0))
        plan = _add(u, capfd, k, values, row_begin=1500, row_end=1500)                      # an empty range
        assert (plan["n"], plan["tiles"], plan["slots"]) == (0, 0, (0, 0))
        plan = _add(u, capfd, keys[:0] if kd else None, values[:0])                          # a column of no rows
        assert (plan["n"], plan["slots"]) == (0, (0, 0))
        _check(u, ref)          # finalize: no rows, or one 0 without key
        if kd:
            assert u.counts_for_keys(keys[:5]).tolist() == [0] * 5
        _add(u, capfd, k, values)
        _check(u, ref.add(k, values))
    finally:
        u.close()


# ---- blocks -----------------------------------------------------------------------------------------------------------------------
def test_the_same_block_twice_changes_nothing(ch, ctx, capfd):
    keys, values = _matrix_block(_rng(10), np.uint16, np.float64)
    ref = UniqExactRef(np.uint16, np.float64).add(keys, values)
    u = ch.UniqExact(np.uint16, np.float64, ctx=ctx)
    try:
        first = _add(u, capfd, keys, values)
        again = _add(u, capfd, keys, values)
        assert again["slots"] == (first["slots"][1],) * 2 and again["holes"] == (first["holes"][1],) * 2 and again["grown"] == 0
        _check(u, ref)
    finally:
        u.close()


@pytest.mark.parametrize("pieces", [1, 2, 7, 64])
def test_one_block_equals_its_pieces(ch, ctx, capfd, pieces):
    keys, values = _matrix_block(_rng(11), np.int32, np.int16)
    ref = UniqExactRef(np.int32, np.int16).add(keys, values)
    kcol, vcol = ctx.upload(keys), ctx.upload(values)
    cuts = np.linspace(0, len(values), pieces + 1).astype(int)
    u = ch.UniqExact(np.int32, np.int16, ctx=ctx)
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            u.add_block(kcol, vcol, row_begin=int(a), row_end=int(b))
        _check(u, ref)
    finally:
        u.close()


def test_finalize_between_blocks_does_not_disturb_later_adds(ch, ctx, capfd):
    rng = _rng(12)
    ref = UniqExactRef(np.uint64, np.uint8)
    u = ch.UniqExact(np.uint64, np.uint8, ctx=ctx)
    try:
        for _ in range(4):
            keys = rng.integers(0, 25, size=1500, dtype=np.uint64)
            values = rng.integers(0, 60, size=1500, dtype=np.uint8)
            u.add_block(keys, values)
            ref.add(keys, values)
            _check(u, ref)
            assert np.array_equal(u.counts_for_keys(np.arange(30, dtype=np.uint64)), ref.counts_for_keys(np.arange(30, dtype=np.uint64)))
            _check(u, ref)   # and finalize twice in a row
    finally:
        u.close()


# ---- LDS stage --------------------------------------------------------------------------------------------------------------------
def test_a_tile_of_one_pair_sends_one_row_on(ch, ctx, capfd):
    keys, values = np.full(TILE, 7, dtype=np.uint64), np.full(TILE, 9, dtype=np.uint64)
    u = ch.UniqExact(np.uint64, np.uint64, ctx=ctx)
    try:
        plan = _add(u, capfd, keys, values)
        assert (plan["tiles"], plan["sent"], plan["lds"], plan["ovf"], plan["slots"]) == (1, 1, TILE - 1, 0, (0, 1))
        plan = _add(u, capfd, np.tile(keys, 3), np.tile(values, 3))       # the set holds the pair now: the look-up settles every row
        assert (plan["found"], plan["sent"], plan["lds"], plan["slots"]) == (3 * TILE, 0, 0, (1, 1))
        _check(u, UniqExactRef(np.uint64, np.uint64).add(keys, values))
    finally:
        u.close()


def test_a_tile_of_distinct_pairs_overflows_the_lds_set(ch, ctx, capfd):
    assert TILE > U.UQ_LDS_CELLS
    rng = _rng(13)
    keys = rng.integers(0, 16, size=TILE, dtype=np.uint64)
    values = rng.permutation(TILE).astype(np.uint64)         # all pairs distinct
    u = ch.UniqExact(np.uint64, np.uint64, ctx=ctx)
    try:
        plan = _add(u, capfd, keys, values)
        assert plan["ovf"] >= TILE - U.UQ_LDS_CELLS and plan["sent"] == TILE and plan["lds"] == 0
        _check(u, UniqExactRef(np.uint64, np.uint64).add(keys, values))
    finally:
        u.close()


def test_more_pairs_on_one_lds_home_cell_than_the_probe_limit(ch, ctx, capfd):
    rng = _rng(14)
    n_pairs, repeat = U.UQ_LDS_PROBES + 24, 10
    k, v = U.pairs_for(rng.integers(0, 5, size=n_pairs, dtype=np.uint64), U.hashes(rng, n_pairs, lds_cell=U.UQ_LDS_CELLS - 3))   # the walk wraps in LDS too
    assert set(U.lds_home(U.uq_hash(k, v)).tolist()) == {U.UQ_LDS_CELLS - 3}
    order = rng.permutation(n_pairs * repeat) % n_pairs
    keys, values = k[order], v[order]
    u = ch.UniqExact(np.uint64, np.uint64, ctx=ctx)
    try:
        plan = _add(u, capfd, keys, values)
        # a pair holds at most one cell, so exactly UQ_LDS_PROBES pairs get one; every row of the other 24 pairs overflows
        assert plan["ovf"] == 24 * repeat and plan["sent"] == U.UQ_LDS_PROBES + 24 * repeat and plan["lds"] == U.UQ_LDS_PROBES * (repeat - 1)
        _check(u, UniqExactRef(np.uint64, np.uint64).add(keys, values))
    finally:
        u.close()


@pytest.mark.parametrize("last", [1, TILE - 1, TILE])
def test_the_last_tile_of_a_block(ch, ctx, capfd, last):
    rng = _rng(15 + last)
    n = TILE + last
    keys = rng.integers(0, 50, size=n, dtype=np.uint16)
    values = rng.integers(0, 50, size=n, dtype=np.uint32)
    keys[-1], values[-1] = 60000, 4000000000        # the block's last row is a pair no other row has
    u = ch.UniqExact(np.uint16, np.uint32, ctx=ctx)
    try:
        plan = _add(u, capfd, keys, values)
        assert plan["tiles"] == 2 and plan["lds"] + plan["sent"] == n
        _check(u, UniqExactRef(np.uint16, np.uint32).add(keys, values))
    finally:
        u.close()


# ---- global table -----------------------------------------------------------------------------------------------------------------
def test_pairs_on_one_global_home_cell(ch, ctx, capfd):
    rng = _rng(16)
    k, v = U.pairs_for(rng.integers(0, 9, size=200, dtype=np.uint64), U.hashes(rng, 200, lg_cap=LG, cell=12345))
    keys, values = np.tile(k, 3), np.tile(v, 3)
    ref = UniqExactRef(np.uint64, np.uint64).add(keys, values)
    u = ch.UniqExact(np.uint64, np.uint64, ctx=ctx)
    try:
        plan = _add(u, capfd, keys, values)
        assert plan["cap"][1] <= 1 << LG and plan["slots"][1] - plan["holes"][1] == 200
        _check(u, ref)
        assert np.array_equal(u.counts_for_keys(np.arange(12, dtype=np.uint64)), ref.counts_for_keys(np.arange(12, dtype=np.uint64)))
    finally:
        u.close()


def test_a_walk_wraps_at_the_end_of_the_smallest_table(ch, ctx, capfd):
    rng = _rng(17)
    cells = np.repeat(np.array([U.UQ_CAP_MIN - 3, U.UQ_CAP_MIN - 2, U.UQ_CAP_MIN - 1], dtype=np.uint64), 20)
    h = np.concatenate([U.hashes(rng, 20, lg_cap=11, cell=c) for c in (U.UQ_CAP_MIN - 3, U.UQ_CAP_MIN - 2, U.UQ_CAP_MIN - 1)])
    assert np.array_equal(U.home(h, U.UQ_CAP_MIN), cells)
    k, v = U.pairs_for(rng.integers(0, 4, size=60, dtype=np.uint64), h)
    u = ch.UniqExact(np.uint64, np.uint64, ctx=ctx)
    try:
        plan = _add(u, capfd, k, v)
        assert plan["cap"] == (U.UQ_CAP_MIN, U.UQ_CAP_MIN) and plan["slots"] == (0, 60)     # 60 pairs on 3 cells: the walks pass cell 0
        ref = UniqExactRef(np.uint64, np.uint64).add(k, v)
        _check(u, ref)
        plan = _add(u, capfd, k[::-1].copy(), v[::-1].copy())                                   # and every one is found again behind the wrap
        assert plan["slots"] == (60, 60)
        _check(u, ref)
    finally:
        u.close()


def test_pairs_that_share_home_and_fingerprint_are_all_kept_and_absent_ones_walk_to_an_empty_cell(ch, ctx, capfd):
    rng = _rng(18)
    fp = 0x5EEDF00D
    h = U.hashes(rng, 12, lg_cap=LG, cell=99, fp=fp)
    assert set(U.fingerprint(h).tolist()) == {fp} and set(U.home(h, U.UQ_CAP_MIN).tolist()) == {99}
    k, v = U.pairs_for(np.array([1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3], dtype=np.uint64), h)
    u = ch.UniqExact(np.uint64, np.uint64, ctx=ctx)
    try:
        plan = _add(u, capfd, k[:8], v[:8])
        assert plan["slots"] == (0, 8)
        ref = UniqExactRef(np.uint64, np.uint64).add(k[:8], v[:8])
        _check(u, ref)                                              # same cell, same fingerprint, different bytes: 8 pairs
        # key 3 is absent: its count is 0, and a pair of key 3 walks past eight cells of its own fingerprint to an empty one
        assert u.counts_for_keys(np.array([3, 1, 2, 77], dtype=np.uint64)).tolist() == [0, 4, 4, 0]
        plan = _add(u, capfd, k[8:9], v[8:9])
        assert plan["slots"] == (8, 9)
        plan = _add(u, capfd, k[:9], v[:9])                          # re-added: found, nothing new
        assert plan["slots"] == (9, 9) and plan["holes"] == (0, 0)
        _check(u, ref.add(k[8:9], v[8:9]))
    finally:
        u.close()


def test_the_look_up_settles_home_cell_hits_and_leaves_the_rest_to_the_tiles(ch, ctx, capfd):
    rng = _rng(25)
    # 300 pairs on 300 different home cells (the same cells in every table up to 2^LG: they stay at home whatever the capacity) ...
    h = np.concatenate([U.hashes(rng, 1, lg_cap=LG, cell=1000 + 3 * i) for i in range(300)])
    k, v = U.pairs_for(rng.integers(0, 7, size=300, dtype=np.uint64), h)
    # ... two pairs on one more cell, added one after the other: the second is displaced to the next cell
    hh = U.hashes(rng, 2, lg_cap=LG, cell=100)
    dk, dv = U.pairs_for(np.array([5, 6], dtype=np.uint64), hh)
    nk, nv = U.pairs_for(rng.integers(0, 7, size=50, dtype=np.uint64), U.hashes(rng, 50, lg_cap=LG, cell=500_000))   # 50 new pairs
    ref = UniqExactRef(np.uint64, np.uint64)
    u = ch.UniqExact(np.uint64, np.uint64, ctx=ctx)
    try:
        plan = _add(u, capfd, k, v)
        assert plan["found"] == 0 and plan["sent"] == 300          # an empty set: no look-up
        _add(u, capfd, dk[:1], dv[:1])
        plan = _add(u, capfd, dk[1:], dv[1:])
        assert (plan["found"], plan["sent"], plan["slots"]) == (0, 1, (301, 302))
        rows_k = np.concatenate([np.tile(k, 4), dk, dk, nk, nk])
        rows_v = np.concatenate([np.tile(v, 4), dv, dv, nv, nv])
        order = rng.permutation(len(rows_k))
        plan = _add(u, capfd, rows_k[order], rows_v[order])
        # at home: the 300 pairs (4 rows each) and the first of the two; the displaced one (2 rows) and the new ones (100 rows) go on
        assert plan["found"] == 4 * 300 + 2 and plan["lds"] + plan["sent"] == 2 + 100 and plan["slots"] == (302, 352) and plan["holes"] == (0, 0)
        _check(u, ref.add(k, v).add(dk, dv).add(nk, nv))
        keep = (rng.integers(0, 2, size=len(rows_k)) * 255).astype(np.uint8)
        plan = _add(u, capfd, rows_k[order], rows_v[order], filter=keep, row_begin=7)   # the filter and the range reach the look-up too
        assert plan["found"] + plan["lds"] + plan["sent"] == int(np.count_nonzero(keep[7:])) and plan["slots"] == (352, 352)
        _check(u, ref)
    finally:
        u.close()


# ---- growth with work in flight ---------------------------------------------------------------------------------------------------
def _distinct_pairs(n):
    i = np.arange(n, dtype=np.uint64)
    return (i % np.uint64(1000)).astype(np.uint32), (i // np.uint64(1000) * np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)


def _sorted_pairs(k, v):
    k, v = np.asarray(k, dtype=np.uint64), np.asarray(v, dtype=np.uint64)
    o = np.lexsort((v, k))
    return k[o], v[o]


def _same_pairs(u, keys, values):
    gk, gv = u.export_pairs()
    gk, gv = _sorted_pairs(gk, gv)
    wk, wv = _sorted_pairs(keys, values)
    return len(gk) == len(wk) and np.array_equal(gk, wk) and np.array_equal(gv, wv) and len(u) == len(wk)


@pytest.mark.parametrize("blocks", [1, 10])
def test_growth_with_rows_deferred(ch, ctx, capfd, blocks):
    n = 300_000
    keys, values = _distinct_pairs(n)
    perm = _rng(19).permutation(n)
    keys, values = keys[perm], values[perm]
    kcol, vcol = ctx.upload(keys), ctx.upload(values)
    u = ch.UniqExact(np.uint32, np.uint64, ctx=ctx, size_hint=0)
    try:
        grown = deferred = 0
        cuts = np.linspace(0, n, blocks + 1).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):
            plan = _add(u, capfd, kcol, vcol, row_begin=int(a), row_end=int(b))
            grown += plan["grown"]
            deferred += plan["deferred"]
            assert plan["rc"] == 0 and plan["cap"][1] >= 2 * int(b) and plan["slots"][1] - plan["holes"][1] == int(b)
            assert _same_pairs(u, keys[:b], values[:b])             # exact after each block
        assert grown >= 2 and deferred > 0
        assert plan["cap"][1] == U.UQ_CAP_MIN * 4 ** 5             # 2048 -> 2^21 cells in x4 steps
        ref = UniqExactRef(np.uint32, np.uint64).add(keys, values)
        _check(u, ref)
        plan = _add(u, capfd, kcol, vcol)                             # every earlier pair re-added: all found
        assert plan["grown"] == 0 and plan["deferred"] == 0 and plan["slots"][0] == plan["slots"][1] and len(u) == n
        assert np.array_equal(u.counts_for_keys(np.arange(1002, dtype=np.uint32)), ref.counts_for_keys(np.arange(1002, dtype=np.uint32)))
    finally:
        u.close()


def test_a_refused_growth_leaves_the_set_as_it_was(ch, capfd):
    c = ch.Context(0)
    try:
        c.set_option("debug", 1)
        c.set_option("test_uniq_fail_growth", 2)      # the second growth of a call answers OOM
        keys, values = _distinct_pairs(40_000)
        u = ch.UniqExact(np.uint32, np.uint64, ctx=c)
        try:
            _add(u, capfd, keys[:900], values[:900])
            _add(u, capfd, keys[:900], values[:900])
            capfd.readouterr()
            with pytest.raises(ch.ChgpuError) as e:
                u.add_block(keys, values)              # 2048 -> 8192 works, 8192 -> 32768 is refused
            assert e.value.code == ch._capi.ERR_OOM
            plan = _ints(_plans(capfd.readouterr().err)[0])
            assert plan["grown"] == 2 and plan["rc"] == ch._capi.ERR_OOM and plan["slots"] == (900, 900)
            assert _same_pairs(u, keys[:900], values[:900])          # exactly what it held before the call
            plan = _add(u, capfd, keys[:4000], values[:4000])       # and a later call works (one growth at most: no refusal)
            assert plan["rc"] == 0
            assert _same_pairs(u, keys[:4000], values[:4000])
        finally:
            u.close()
    finally:
        c.close()


# ---- the same new pairs from many workgroups at once ------------------------------------------------------------------------------
def test_the_same_new_pairs_from_many_workgroups(ch, ctx, capfd):
    rng = _rng(20)
    pk = rng.integers(0, 20, size=1000, dtype=np.uint64)
    pv = rng.permutation(1000).astype(np.uint64) * np.uint64(0x100000001B3)
    idx = np.concatenate([rng.permutation(TILE) % 1000 for _ in range(64)])       # every tile holds every pair
    keys, values = pk[idx], pv[idx]
    ref = UniqExactRef(np.uint64, np.uint64).add(pk, pv)
    assert len(ref) == 1000
    u = ch.UniqExact(np.uint64, np.uint64, ctx=ctx, size_hint=4096)
    try:
        plan = _add(u, capfd, keys, values)
        assert plan["tiles"] == 64 and plan["sent"] >= 64 * 1000 and plan["lds"] + plan["sent"] == 64 * TILE
        assert plan["slots"][1] - plan["holes"][1] == 1000 and plan["slots"][1] >= 1000
        assert len(u) == 1000
        _check(u, ref)          # each pair exported once, holes skipped
    finally:
        u.close()


# ---- merge, export_pairs, counts_for_keys -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True], ids=["disjoint", "overlapping"])
@pytest.mark.parametrize("kd", [np.int16, None], ids=["keyed", "nokey"])
def test_merge_is_union_and_leaves_src_usable(ch, ctx, capfd, kd, overlap):
    rng = _rng(21)
    keys, values = _matrix_block(rng, kd, np.float32, n=6000)
    cut_a, cut_b = (4000, 2000) if overlap else (3000, 3000)
    ka, kb = (keys[:cut_a], keys[cut_b:]) if kd else (None, None)
    a, b = ch.UniqExact(kd, np.float32, ctx=ctx), ch.UniqExact(kd, np.float32, ctx=ctx)
    try:
        a.add_block(ka, values[:cut_a])
        b.add_block(kb, values[cut_b:])
        ref_b = UniqExactRef(kd, np.float32).add(kb, values[cut_b:])
        capfd.readouterr()
        a.merge(b)
        plan = _ints(_plans(capfd.readouterr().err)[0])
        assert plan["plan"] == "merge" and plan["rc"] == 0
        _check(a, UniqExactRef(kd, np.float32).add(keys, values))
        _check(b, ref_b)                                             # src unchanged ...
        b.add_block(ka, values[:cut_a])                              # ... and usable
        _check(b, UniqExactRef(kd, np.float32).add(keys, values))
        a.merge(a)
        assert len(a) == len(b)
    finally:
        a.close()
        b.close()


def test_exported_pairs_re_added_give_the_same_set(ch, ctx, capfd):
    keys, values = _matrix_block(_rng(22), np.uint32, np.float64)
    ref = UniqExactRef(np.uint32, np.float64).add(keys, values)
    u, w = ch.UniqExact(np.uint32, np.float64, ctx=ctx), ch.UniqExact(np.uint32, np.float64, ctx=ctx)
    shards = [ch.UniqExact(np.uint32, np.float64, ctx=ctx) for _ in range(2)]
    try:
        u.add_block(keys, values)
        kc, vc = u.export_pair_columns()
        assert kc.dtype == np.uint32 and vc.dtype == np.float64 and kc.size() == len(ref)
        w.add_block(kc, vc)          # columns stay in HBM: the peer's add_block
        _check(w, ref)
        # a sharded GROUP BY routes the pairs by key with the existing exchange: the shards' sets are disjoint by key and add up
        (pk, pv), counts = ch.partition_by_hash(kc, 2, [kc, vc])
        assert int(counts.sum()) == len(ref)
        edge = 0
        for sh, cnt in zip(shards, counts.tolist()):
            sh.add_block(pk, pv, row_begin=edge, row_end=edge + cnt)
            edge += cnt
        fins = [dict(zip(*[x.tolist() for x in sh.finalize()])) for sh in shards]
        assert not set(fins[0]) & set(fins[1])
        assert {**fins[0], **fins[1]} == ref.finalize()
    finally:
        for x in [u, w] + shards:
            x.close()


def test_counts_for_keys_lines_up_with_an_aggregator_finalize(ch, ctx, capfd):
    rng = _rng(23)
    n = 5000
    keys = rng.integers(0, 40, size=n, dtype=np.uint32)
    a = rng.integers(-100, 100, size=n, dtype=np.int64)
    x = rng.integers(0, 25, size=n, dtype=np.int32)
    cond = (rng.integers(0, 3, size=n) != 0).astype(np.uint8) * np.uint8(255)
    cond[keys == 17] = 0                           # every row of key 17 is masked out of the distinct count
    assert np.any(keys == 17)
    agg = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)], ctx=ctx)
    u = ch.UniqExact(np.uint32, np.int32, ctx=ctx)
    try:
        agg.execute_on_block(keys, [a, None])
        u.add_block(keys, x, filter=cond)
        gk, _ = agg.finalize_columns()
        got = u.counts_for_keys(gk)              # the key Column of the aggregator's result, still in HBM
        ref = UniqExactRef(np.uint32, np.int32).add(keys, x, filter=cond)
        gkeys = gk.numpy()
        assert sorted(gkeys.tolist()) == sorted(set(keys.tolist()))
        assert np.array_equal(got, ref.counts_for_keys(gkeys))
        assert got[gkeys == 17].tolist() == [0] and 17 not in ref.finalize()       # uniqExactIf of a group with no row: 0
    finally:
        agg.close()
        u.close()


def test_keydict_ids_and_packed_keys_are_ordinary_keys(ch, ctx, capfd):
    rng = _rng(24)
    n = 4000
    c0 = rng.integers(0, 6, size=n, dtype=np.uint64)
    c1 = rng.integers(0, 5, size=n, dtype=np.uint64)
    c2 = rng.integers(0, 3, size=n, dtype=np.uint16)
    x = rng.integers(0, 12, size=n, dtype=np.int64)
    # keys128: ids of the wide-key dictionary are a UInt32 key column
    d = ch.KeyDict([np.uint64, np.uint64, np.uint16], ctx=ctx)
    ids = d.encode([c0, c1, c2])
    u = ch.UniqExact(np.uint32, np.int64, ctx=ctx)
    try:
        u.add_block(ids, x)
        ids_np = ids.numpy()
        ref = UniqExactRef(np.uint32, np.int64).add(ids_np, x)
        _check(u, ref)
        want = {}
        for t in set(zip(c0.tolist(), c1.tolist(), c2.tolist(), x.tolist())):
            want[t[:3]] = want.get(t[:3], 0) + 1
        k, c = u.finalize_columns()
        back = [col.numpy() for col in d.key_columns(k)]
        assert dict(zip(zip(*[b.tolist() for b in back]), c.numpy().tolist())) == want
    finally:
        u.close()
    # packed keys (UInt32 + UInt16 + UInt8 in one UInt64)
    p0, p1, p2 = c0.astype(np.uint32), c2, c1.astype(np.uint8)
    packed = ch.pack_fixed_keys([ctx.upload(p0), ctx.upload(p1), ctx.upload(p2)])
    u = ch.UniqExact(np.uint64, np.int64, ctx=ctx)
    try:
        u.add_block(packed, x)
        _check(u, UniqExactRef(np.uint64, np.int64).add(packed.numpy(), x))
        want = {}
        for t in set(zip(p0.tolist(), p1.tolist(), p2.tolist(), x.tolist())):
            want[t[:3]] = want.get(t[:3], 0) + 1
        assert sorted(u.finalize()[1].tolist()) == sorted(want.values())
    finally:
        u.close()


# ---- entry checks -----------------------------------------------------------------------------------------------------------------
def test_entry_checks_return_their_codes_and_leave_the_set_usable(ch, ctx, capfd):
    import ctypes as C
    K = ch._capi
    keys = np.arange(100, dtype=np.uint32)
    values = np.arange(100, dtype=np.int64)
    kcol, vcol = ctx.upload(keys), ctx.upload(values)
    u = ch.UniqExact(np.uint32, np.int64, ctx=ctx)
    nokey = ch.UniqExact(None, np.int64, ctx=ctx)
    other = ch.UniqExact(np.uint32, np.int32, ctx=ctx)

    def code(fn, *a, **kw):
        with pytest.raises(ch.ChgpuError) as e:
            fn(*a, **kw)
        return e.value.code, str(e.value)

    try:
        u.add_block(kcol, vcol)
        assert code(u.add_block, ctx.upload(keys.astype(np.uint64)), vcol)[0] == K.ERR_BAD_ARGUMENTS          # key type
        assert code(u.add_block, kcol, ctx.upload(values.astype(np.int32)))[0] == K.ERR_BAD_ARGUMENTS          # value type
        assert code(u.add_block, kcol, vcol, filter=ctx.upload(np.ones(100, dtype=np.uint16)))[0] == K.ERR_BAD_ARGUMENTS
        assert code(u.add_block, kcol, vcol, row_begin=6, row_end=5)[0] == K.ERR_BAD_ARGUMENTS
        assert code(u.add_block, kcol, vcol, row_begin=0, row_end=101)[0] == K.ERR_BAD_ARGUMENTS
        assert code(u.add_block, ctx.upload(keys[:99]), vcol)[0] == K.ERR_SIZES_MISMATCH
        assert code(u.add_block, kcol, vcol, filter=np.ones(99, dtype=np.uint8))[0] == K.ERR_SIZES_MISMATCH
        c, msg = code(u.add_block, None, vcol)
        assert c == K.ERR_BAD_ARGUMENTS and "NULL" in msg
        assert code(u.merge, other)[0] == K.ERR_BAD_ARGUMENTS and code(u.merge, nokey)[0] == K.ERR_BAD_ARGUMENTS
        assert code(u.counts_for_keys, keys.astype(np.uint64))[0] == K.ERR_BAD_ARGUMENTS
        assert code(nokey.counts_for_keys, keys)[0] == K.ERR_BAD_ARGUMENTS
        assert code(ch.UniqExact, np.uint32, np.int64, ctx=ctx, size_hint=2**31 + 1)[0] == K.ERR_TOO_MANY_ROWS
        h = C.c_void_p()
        assert K.lib().chgpu_uniq_create(ctx._h, 77, K.I64, 0, C.byref(h)) == K.ERR_BAD_ARGUMENTS
        assert K.lib().chgpu_uniq_create(ctx._h, K.U32, 77, 0, C.byref(h)) == K.ERR_BAD_ARGUMENTS
        # NULL outputs on a live handle
        n = C.c_uint64(0)
        a, b = C.c_void_p(), C.c_void_p()
        for rc in (K.lib().chgpu_uniq_size(u._h, None), K.lib().chgpu_uniq_finalize(u._h, None, C.byref(b), C.byref(n)),
                   K.lib().chgpu_uniq_finalize(u._h, C.byref(a), None, C.byref(n)), K.lib().chgpu_uniq_export_pairs(u._h, C.byref(a), C.byref(b), None),
                   K.lib().chgpu_uniq_export_pairs(u._h, None, C.byref(b), C.byref(n)), K.lib().chgpu_uniq_counts_for_keys(u._h, kcol._h, None),
                   K.lib().chgpu_uniq_merge(u._h, None), K.lib().chgpu_uniq_create(ctx._h, K.U32, K.I64, 0, None)):
            assert rc == K.ERR_BAD_ARGUMENTS and b"NULL" in K.lib().chgpu_last_error()
        # without key: keys_out may be NULL
        assert K.lib().chgpu_uniq_finalize(nokey._h, None, C.byref(b), C.byref(n)) == K.OK and n.value == 1
        K.lib().chgpu_col_free(b)
        # nothing above changed the set
        _check(u, UniqExactRef(np.uint32, np.int64).add(keys, values))
    finally:
        u.close()
        nokey.close()
        other.close()
