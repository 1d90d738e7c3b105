"""The ASOF join (asof_kernels.hip: k_asof_stage, the filter / concat / two stable sorts / gather of asof_build, k_asof_probe) at the edges
of its code, row for row against tests/asof_ref.py (a stable sort and np.searchsorted on values in their own dtype; test_asof_ref.py
holds it against oracle.asof_pairs).

Every comparison is exact equality of (left_row, block, row); the header of asof_kernels.hip is the contract, its tie rule included (equal
(key, asof) build rows: the last inserted for >= / >, the first inserted for <= / <).  Each test that generates inputs asserts on the
REFERENCE's output that the rows it is about exist (a miss at the wrapped position, a winner in the middle of a block, ...): a test that
passes because nothing reached the branch fails instead."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asof_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GE, GT, LE, LT = R.ASOF_GREATER_OR_EQUALS, R.ASOF_GREATER, R.ASOF_LESS_OR_EQUALS, R.ASOF_LESS
INEQS = [GE, GT, LE, LT]
INEQ_IDS = [">=", ">", "<=", "<"]
U8 = np.uint8


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    return ch.Context(0)


def _num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def surviving(build):
    n = 0
    for keys, t, nm, jm in build:
        keep = np.ones(keys.shape[0], dtype=bool)
        if nm is not None:
            keep &= nm == 0
        if jm is not None:
            keep &= jm != 0
        if t.dtype.kind == "f":
            keep &= ~np.isnan(t)
        n += int(keep.sum())
    return n


def make_join(ch, ctx, build, ineq, left):
    """a join over `build`: add_block counts every block, total_rows only the surviving rows"""
    key_dt, asof_dt = build[0][0].dtype, build[0][1].dtype
    j = ch.AsofJoin(ch.JOIN_LEFT if left else ch.JOIN_INNER, ineq, key_dtype=key_dt, asof_dtype=asof_dt, ctx=ctx)
    for i, (keys, t, nm, jm) in enumerate(build):
        assert keys.dtype == key_dt and t.dtype == asof_dt
        assert j.add_block(keys, t, nm, jm) == i
    assert j.total_rows == surviving(build)
    return j


def check_probe(j, build, lk, lt, ineq, left, lnm=None, what=None):
    """probe `j` and compare with the reference; -> the reference's (left_row, block, row)"""
    assert lk.dtype == build[0][0].dtype and lt.dtype == build[0][1].dtype
    got = j.joined_pairs(lk, lt, lnm)
    want = R.asof_ref(build, lk, lt, ineq, lnm, left)
    assert all(x.dtype == np.int64 for x in got)
    d = R.first_difference(got, want)
    assert d is None, (what, INEQ_IDS[INEQS.index(ineq)], "LEFT" if left else "INNER", d)
    assert j.total_rows == surviving(build)
    return want


def check(ch, ctx, build, lk, lt, ineq, lnm=None, what=None):
    """INNER and LEFT over fresh joins; -> the LEFT reference (block, row) per left row.  INNER is LEFT without its default rows."""
    wi = check_probe(make_join(ch, ctx, build, ineq, False), build, lk, lt, ineq, False, lnm, what)
    wl = check_probe(make_join(ch, ctx, build, ineq, True), build, lk, lt, ineq, True, lnm, what)
    m = wl[1] >= 0
    assert np.array_equal(wl[0], np.arange(lk.shape[0])) and np.array_equal(wi[0], wl[0][m]) and np.array_equal(wi[1], wl[1][m])
    assert np.array_equal(wl[1] < 0, wl[2] < 0)
    return wl[1], wl[2]


def winners(build, block, row, col):
    """column `col` (0: key, 1: asof) of the build rows a LEFT answer names; only meaningful where block >= 0"""
    out = np.zeros(block.shape[0], dtype=build[0][col].dtype)
    for b, blk in enumerate(build):
        m = block == b
        out[m] = blk[col][row[m]]
    return out


def split(keys, t, cut):
    return [(keys[:cut], t[:cut], None, None), (keys[cut:], t[cut:], None, None)]


def key_of_bits(dtype, bits):
    """keys of `dtype` with the given zero-extended bit patterns"""
    dt = np.dtype(dtype)
    return np.array(bits, dtype=np.dtype(f"u{dt.itemsize}")).view(dt)


def test_the_constants_agree(ch):
    for name, value in R.INEQUALITIES.items():
        assert getattr(ch, "ASOF_" + name) == value


# ------------------------------------------------------------------------------------------------------------------------------
# a. every asof type at its extremes
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.ASOF_TYPES, ids=lambda d: np.dtype(d).name)
def test_every_asof_type_at_its_extremes(ch, ctx, dtype):
    dt = np.dtype(dtype)
    rng = np.random.Generator(np.random.PCG64(500 + dt.num))
    pool = R.value_pool(dt)                       # ascending; floats: -0.0 and +0.0 are the only equal pair, NaN comes last
    lo, hi = pool[0], pool[-2] if dt.kind == "f" else pool[-1]
    present = np.array([3, 10, 2**40 + 1], dtype=np.uint64)
    absent = np.array([5, 2**63 + 7], dtype=np.uint64)
    order = rng.permutation(3 * pool.shape[0])
    build = split(np.repeat(present, pool.shape[0])[order], np.tile(pool, 3)[order], order.shape[0] // 2 + 1)
    lk = np.repeat(np.concatenate([present, absent]), pool.shape[0])
    lt = np.tile(pool, 5)
    there = np.isin(lk, present)
    nan = np.isnan(lt) if dt.kind == "f" else np.zeros(lt.shape[0], dtype=bool)
    zero_meets_plus_zero = set()
    for ineq in INEQS:
        block, row = check(ch, ctx, build, lk, lt, ineq, what=dt.name)
        hit = block >= 0
        pv = winners(build, block, row, 1)
        assert hit.any() and not hit[~there].any() and np.array_equal(winners(build, block, row, 0)[hit], lk[hit])
        at_lo, at_hi = there & (lt == lo), there & (lt == hi)
        assert at_lo.sum() == 3 and at_hi.sum() == 3
        # the type's minimum has nothing below it and its maximum nothing above; every other extreme probe finds its partner
        assert not hit[at_lo].any() if ineq == GT else (hit[at_lo].all() and ((pv[at_lo] > lo).all() if ineq == LT else (pv[at_lo] == lo).all()))
        assert not hit[at_hi].any() if ineq == LT else (hit[at_hi].all() and ((pv[at_hi] < hi).all() if ineq == GT else (pv[at_hi] == hi).all()))
        if dt.kind == "f":
            assert nan.sum() == 5 and not hit[nan].any()        # default rows under LEFT, and `check` saw them absent under INNER
            mz = there & (lt == 0) & np.signbit(lt)
            assert mz.sum() == 3 and hit[mz].all()
            if ineq in (GE, LE):
                assert (pv[mz] == 0).all()
                if (~np.signbit(pv[mz])).any():
                    zero_meets_plus_zero.add(ineq)
            else:                                               # -0.0 is neither above nor below +0.0: the next subnormal
                assert (pv[mz] == (-1 if ineq == GT else 1) * np.finfo(dt).smallest_subnormal).all()
    assert dt.kind != "f" or zero_meets_plus_zero == {GE, LE}


# ------------------------------------------------------------------------------------------------------------------------------
# b. every key type and the ends of the sorted array
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_dtype", R.KEY_TYPES, ids=lambda d: np.dtype(d).name)
def test_every_key_type_and_absent_keys_around_the_present_ones(ch, ctx, key_dtype):
    dt = np.dtype(key_dtype)
    rng = np.random.Generator(np.random.PCG64(600 + dt.num))
    ones = (1 << (8 * dt.itemsize)) - 1
    half = 1 << (8 * dt.itemsize - 1)               # the sign bit: signed types order their negative keys ABOVE the others here
    present = key_of_bits(dt, [5, half - 3, half + 2, ones - 4])
    absent = key_of_bits(dt, [2, half, ones - 1])   # below every present key, between two of them, above all of them
    per_key = 40
    t = np.concatenate([rng.choice(1_000_000, size=per_key, replace=False) for _ in present]).astype(np.uint32) + np.uint32(1000)
    order = rng.permutation(t.shape[0])
    build = split(np.repeat(present, per_key)[order], t[order], 70)
    probes = np.concatenate([[0, 999, 2**32 - 1], rng.integers(0, 1_002_000, size=30)]).astype(np.uint32)
    lk = np.repeat(np.concatenate([present, absent]), probes.shape[0])
    lt = np.tile(probes, 7)
    there = np.isin(lk, present)
    for ineq in INEQS:
        block, row = check(ch, ctx, build, lk, lt, ineq, what=dt.name)
        hit = block >= 0
        assert not hit[~there].any() and (~there).sum() == 3 * probes.shape[0]
        assert hit[there].sum() > 50 and (~hit[there]).sum() >= 4
        assert np.array_equal(winners(build, block, row, 0)[hit], lk[hit])


@pytest.mark.parametrize("key_dtype", R.KEY_TYPES, ids=lambda d: np.dtype(d).name)
def test_key_bits_zero_and_all_ones_at_the_ends_of_the_search(ch, ctx, key_dtype):
    dt = np.dtype(key_dtype)
    rng = np.random.Generator(np.random.PCG64(700 + dt.num))
    ones = (1 << (8 * dt.itemsize)) - 1
    present = key_of_bits(dt, [0, 7, ones - 3, ones])
    assert dt.kind == "u" or present[-1] == -1
    values = np.arange(100, 200, 10, dtype=np.uint32)
    order = rng.permutation(4 * values.shape[0])
    build = split(np.repeat(present, values.shape[0])[order], np.tile(values, 4)[order], 17)
    #            lo == 0  match    match    front of key 7     lo == nb    match        match        behind key ones - 3        absent
    bits = [0,       0,       0,       7,       7,        ones,       ones,        ones,        ones - 3,    ones - 3,      3,   ones - 1]
    lt = np.array([50, 105,     100,     50,      105,      1000,       185,         190,         1000,        185,           150, 150], dtype=np.uint32)
    lk = key_of_bits(dt, bits)
    for ineq in INEQS:
        block, row = check(ch, ctx, build, lk, lt, ineq, what=dt.name)
        hit = block >= 0
        assert np.array_equal(winners(build, block, row, 0)[hit], lk[hit]) and not hit[10:].any()
        pv = winners(build, block, row, 1)
        if ineq in (GE, GT):
            # (key 0, 50): the bound is entry 0 and the position in front of it wraps; (key 7, 50): the entry in front belongs to key 0
            assert not hit[0] and not hit[3] and hit[1] and pv[1] == 100 and hit[4] and pv[4] == 100
            assert hit[5] and pv[5] == 190 and hit[8] and pv[8] == 190
            assert pv[2] == 100 if ineq == GE else not hit[2]
        else:
            # (key ones, 1000): the bound is nb; (key ones - 3, 1000): the entry at the bound belongs to key ones
            assert not hit[5] and not hit[8] and hit[6] and pv[6] == 190 and hit[9] and pv[9] == 190
            assert hit[0] and pv[0] == 100 and hit[3] and pv[3] == 100
            assert pv[7] == 190 if ineq == LE else not hit[7]


@pytest.mark.parametrize("key_dtype", [np.float32, np.float64])
def test_float_keys_are_not_implemented(ch, ctx, key_dtype):
    for kind in (ch.JOIN_INNER, ch.JOIN_LEFT):
        with pytest.raises(ch.ChgpuError) as e:
            ch.AsofJoin(kind, key_dtype=key_dtype, asof_dtype=np.uint32, ctx=ctx)
        assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED


# ------------------------------------------------------------------------------------------------------------------------------
# c. ties follow the stated rule
# ------------------------------------------------------------------------------------------------------------------------------
TIE_POOL = np.array([-5, 0, 7, 7000, 1234], dtype=np.int32)
BIG_KEY, BIG_VALUE = 77, 1234


def tie_build():
    """blocks 0 and 3: four keys over five values, so every (key, value) has many copies inside each block and in both; block 1 is empty,
    block 2 fully masked.  Blocks 4 and 5: 3001 + 1098 copies of (77, 1234) on the odd rows, other keys in between; the first copy is
    NULL and the last one has a zero ON mask, which leaves 4097 equal rows: one more than the 4096-row tile of the sort."""
    rng = np.random.Generator(np.random.PCG64(800))

    def small(n):
        return rng.integers(0, 4, size=n).astype(np.uint32), TIE_POOL[rng.integers(0, TIE_POOL.shape[0], size=n)]

    def big(copies):
        n = 2 * copies + 2
        keys = (100 + (np.arange(n) // 2) % 5).astype(np.uint32)
        t = TIE_POOL[rng.integers(0, TIE_POOL.shape[0], size=n)]
        keys[1:2 * copies:2], t[1:2 * copies:2] = BIG_KEY, BIG_VALUE
        assert (keys == BIG_KEY).sum() == copies and keys[0] != BIG_KEY and keys[-1] != BIG_KEY and keys[-2] != BIG_KEY
        return keys, t

    k0, t0 = small(300)
    k2, t2 = small(200)
    k3, t3 = small(300)
    k4, t4 = big(3001)
    k5, t5 = big(1098)
    nm4 = np.zeros(k4.shape[0], dtype=U8)
    nm4[1] = 1
    jm5 = np.ones(k5.shape[0], dtype=U8)
    jm5[2 * 1098 - 1] = 0
    e = np.zeros(0, dtype=np.uint32)
    # blocks 0 and 3 lose three rows in ten: block 0 through its null map for keys 0, 1 and its ON mask for keys 2, 3; block 3 the other way
    drop0, drop3 = rng.random(300) < 0.3, rng.random(300) < 0.3
    nm0, jm0 = (drop0 & (k0 < 2)).astype(U8), (~(drop0 & (k0 >= 2))).astype(U8)
    nm3, jm3 = (drop3 & (k3 >= 2)).astype(U8), (~(drop3 & (k3 < 2))).astype(U8)
    build = [(k0, t0, nm0, jm0), (e, e.astype(np.int32), None, None), (k2, t2, None, np.zeros(200, dtype=U8)),
             (k3, t3, nm3, jm3), (k4, t4, nm4, None), (k5, t5, None, jm5)]
    copies = sum(int(((k == BIG_KEY) & (t == BIG_VALUE) & (nm is None or nm == 0) & (jm is None or jm != 0)).sum()) for k, t, nm, jm in build)
    assert copies == 4097
    return build


def test_ties_follow_the_stated_rule(ch, ctx):
    build = tie_build()
    unmasked = [(k, t, None, None) if b != 2 else (k, t, nm, jm) for b, (k, t, nm, jm) in enumerate(build)]
    keys = np.array([0, 1, 2, 3, BIG_KEY, 100, 101, 102, 103, 104, 50], dtype=np.uint32)
    values = (TIE_POOL[:, None] + np.array([-1, 0, 1], dtype=np.int32)[None, :]).ravel()
    lk, lt = np.repeat(keys, values.shape[0]), np.tile(values, keys.shape[0])
    for ineq in INEQS:
        block, row = check(ch, ctx, build, lk, lt, ineq)
        hit = block >= 0
        assert not hit[lk == 50].any() and hit[lk != 50].any()
        # the 4097 equal rows: the last surviving copy sits in the later block, the first in the earlier one, neither at an end of its block
        probe = {GE: 1234, GT: 1235, LE: 1234, LT: 1233}[ineq]
        at = np.flatnonzero((lk == BIG_KEY) & (lt == probe))
        assert at.shape[0] == 1
        want = (5, 2 * 1098 - 3) if ineq in (GE, GT) else (4, 3)
        assert (int(block[at[0]]), int(row[at[0]])) == want and 0 < want[1] < build[want[0]][0].shape[0] - 1
        # ties inside a block and across blocks 0 and 3, over the empty and the fully masked block between them
        first, last = (block == 0) & (lk < 4), (block == 3) & (lk < 4)
        assert (last.sum() > 10 and first.sum() < last.sum()) if ineq in (GE, GT) else (first.sum() > 10 and last.sum() < first.sum())
        assert (row[first | last] > 0).any() and not (block == 1).any() and not (block == 2).any()
        # a copy removed by a null map or an ON mask: without the masks another copy of the SAME (key, value) would have won
        b0, r0 = R.asof_ref(unmasked, lk, lt, ineq, None, True)[1:]
        moved = hit & ((b0 != block) | (r0 != row))
        same = moved & (winners(build, block, row, 1) == winners(build, b0, r0, 1))
        # (>= / >: the last copy went, from block 3 or 5; <= / <: the first, from block 0 or 4; which mask took it depends on the key)
        later = ineq in (GE, GT)
        assert np.isin(b0[same], [3, 5] if later else [0, 4]).all()
        by_null_map = same & ((lk >= 2) & (lk < 4) if later else lk < 2)
        by_join_mask = same & (lk < 2 if later else (lk >= 2) & (lk < 4))
        assert by_null_map.any() and by_join_mask.any(), (by_null_map.sum(), by_join_mask.sum())


# ------------------------------------------------------------------------------------------------------------------------------
# d. blocks, masks and row ids
# ------------------------------------------------------------------------------------------------------------------------------
def test_block_and_row_ids_with_both_masks_on_one_block(ch, ctx):
    rng = np.random.Generator(np.random.PCG64(900))
    n = 64
    keys = rng.integers(0, 3, size=n).astype(np.uint16)
    t = rng.permutation(n).astype(np.int16) * np.int16(10)          # no ties: every probe below names one row
    nm = (np.arange(n) % 4 == 1) | (np.arange(n) % 4 == 3)
    jm = ~((np.arange(n) % 4 == 2) | (np.arange(n) % 4 == 3))
    assert (nm & jm).any() and (~nm & ~jm).any() and (nm & ~jm).any() and (~nm & jm).any()   # only NULL, only ON, both, neither
    e = np.zeros(0, dtype=np.uint16)
    k5, t5 = np.array([0, 1, 2, 0, 1], dtype=np.uint16), np.array([-7, -7, -7, 5, 5], dtype=np.int16)
    build = [(k5, t5, None, None), (e, e.astype(np.int16), None, None), (k5, t5 + np.int16(1), np.ones(5, dtype=U8), None),
             (keys, t, nm.astype(U8), jm.astype(U8)), (k5, t5 + np.int16(2), None, np.zeros(5, dtype=U8))]
    assert surviving(build) == 5 + n // 4
    # every row of block 3 is probed at its own value: a masked row is then the best partner under >= and <=, and must not be one
    lk, lt = np.concatenate([keys, k5, np.array([7], dtype=np.uint16)]), np.concatenate([t, t5, np.array([5], dtype=np.int16)])   # key 7 is absent
    no_join_mask = [blk if b != 3 else (keys, t, nm.astype(U8), None) for b, blk in enumerate(build)]
    no_null_map = [blk if b != 3 else (keys, t, None, jm.astype(U8)) for b, blk in enumerate(build)]
    for ineq in INEQS:
        block, row = check(ch, ctx, build, lk, lt, ineq)
        hit = block >= 0
        assert set(block[hit].tolist()) == {0, 3} and hit.any() and not hit.all()
        kept = np.flatnonzero(~nm & jm)
        assert np.isin(row[block == 3], kept).all()
        rank = np.searchsorted(kept, row[block == 3])                     # where the row sits among the surviving rows of its block
        assert (rank != row[block == 3]).sum() > 5
        for other in (no_join_mask, no_null_map):                         # each mask alone would have given other partners
            bo, ro = R.asof_ref(other, lk, lt, ineq, None, True)[1:]
            assert ((bo != block) | (ro != row)).any()


def test_twelve_one_row_blocks(ch, ctx):
    t = np.array([50, 10, 30, 30, 20, 60, 10, 40, 30, 5, 70, 20], dtype=np.uint8)
    keys = np.array([1, 1, 1, 2, 1, 1, 2, 1, 1, 2, 1, 2], dtype=np.int8)
    build = [(keys[i:i + 1], t[i:i + 1], None, None) for i in range(12)]
    probes = np.arange(0, 80, 5, dtype=np.uint8)
    lk, lt = np.repeat(np.array([1, 2, 3], dtype=np.int8), probes.shape[0]), np.tile(probes, 3)
    for ineq in INEQS:
        block, row = check(ch, ctx, build, lk, lt, ineq)
        hit = block >= 0
        assert (row[hit] == 0).all() and len(set(block[hit].tolist())) >= 8 and not hit[lk == 3].any() and not hit[lk != 3].all()
        at = np.flatnonzero((lk == 1) & (lt == {GE: 30, GT: 35, LE: 30, LT: 25}[ineq]))[0]
        assert block[at] == (8 if ineq in (GE, GT) else 2)                # value 30 of key 1 sits in blocks 2 and 8 (and key 2's in block 3)


def test_only_the_last_block_survives(ch, ctx):
    rng = np.random.Generator(np.random.PCG64(910))
    blocks = []
    for n in (40, 30, 50):
        blocks.append((rng.integers(0, 3, size=n).astype(np.uint64), (rng.permutation(200)[:n] * 3).astype(np.uint64)))
    build = [(blocks[0][0], blocks[0][1], np.ones(40, dtype=U8), None), (blocks[1][0], blocks[1][1], None, np.zeros(30, dtype=U8)),
             (blocks[2][0], blocks[2][1], None, None)]
    lk = np.concatenate([b[0] for b in blocks])
    lt = np.concatenate([b[1] for b in blocks])
    for ineq in INEQS:
        block, row = check(ch, ctx, build, lk, lt, ineq)
        assert set(block.tolist()) == {-1, 2} and (block == 2).sum() > 60
        unmasked = R.asof_ref([(k, t, None, None) for k, t in blocks], lk, lt, ineq, None, True)
        assert (unmasked[1] == 0).any() and (unmasked[1] == 1).any()


@pytest.mark.parametrize("asof_dtype", [np.uint32, np.int64, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_every_row_of_every_block_masked_out(ch, ctx, asof_dtype):
    """rows == 0 with blocks that were not empty: the probe runs over no sorted array at all"""
    dt = np.dtype(asof_dtype)
    keys = np.array([1, 2, 3, 1, 2, 3, 1], dtype=np.uint32)
    t = np.full(7, np.nan, dtype=dt) if dt.kind == "f" else np.arange(7).astype(dt)
    if dt.kind == "f":
        build = [(keys, t, None, None), (keys[:3], t[:3], None, np.ones(3, dtype=U8))]
    else:
        build = [(keys, t, np.ones(7, dtype=U8), None), (keys[:3], t[:3], None, np.zeros(3, dtype=U8)),
                 (keys, t, (np.arange(7) % 2).astype(U8), (np.arange(7) % 2).astype(U8))]
    assert surviving(build) == 0
    lk = np.tile(np.array([1, 2, 3, 4], dtype=np.uint32), 70)            # 280 rows: more than one workgroup
    lt = (np.arange(280) % 9).astype(dt)
    for ineq in INEQS:
        block, row = check(ch, ctx, build, lk, lt, ineq)
        assert (block == -1).all() and (row == -1).all()
        j = make_join(ch, ctx, build, ineq, False)
        assert j.total_rows == 0
        l, b, r = j.joined_pairs(lk, lt)
        assert l.shape == b.shape == r.shape == (0,) and j.total_rows == 0


# ------------------------------------------------------------------------------------------------------------------------------
# e. sizes around the search and the workgroup
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ineq", INEQS, ids=INEQ_IDS)
def test_every_bound_position_of_small_builds(ch, ctx, ineq):
    for nb in (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025):
        t = 2 * np.arange(nb, dtype=np.int32)
        build = [(np.full(nb, 9, dtype=np.uint32), t, None, None)]
        lt = np.arange(-1, 2 * nb + 1, dtype=np.int32)                    # every value, every gap, below the first and above the last
        lk = np.full(lt.shape[0], 9, dtype=np.uint32)
        block, row = check(ch, ctx, build, lk, lt, ineq, what=nb)
        hit = block >= 0
        misses = {GE: lt < 0, GT: lt <= 0, LE: lt > t[-1], LT: lt >= t[-1]}[ineq]
        assert np.array_equal(~hit, misses) and set(row[hit].tolist()) == set(range(nb))


@pytest.mark.parametrize("ineq", INEQS, ids=INEQ_IDS)
def test_every_bound_position_over_fifty_keys(ch, ctx, ineq):
    nb = 257
    t = 2 * np.arange(nb, dtype=np.int32)
    keys = (np.arange(nb) % 50).astype(np.uint32)
    build = [(keys, t, None, None)]
    values = np.arange(-1, 2 * nb + 1, dtype=np.int32)
    lk, lt = np.repeat(np.arange(51, dtype=np.uint32), values.shape[0]), np.tile(values, 51)
    block, row = check(ch, ctx, build, lk, lt, ineq)
    hit = block >= 0
    assert not hit[lk == 50].any() and set(row[hit].tolist()) == set(range(nb))
    assert all((~hit[lk == k]).any() and hit[lk == k].any() for k in range(50))
    assert np.array_equal(keys[row[hit]], lk[hit])


def test_probe_lengths_against_one_handle(ch, ctx):
    rng = np.random.Generator(np.random.PCG64(920))
    nb = 700
    keys = rng.integers(0, 5, size=nb).astype(np.uint8)
    t = rng.permutation(4000)[:nb].astype(np.uint16)
    build = split(keys, t, 333)
    for ineq in INEQS:
        for left in (False, True):
            j = make_join(ch, ctx, build, ineq, left)
            for n in (257, 0, 1, 255, 256, 0, 257, 1):
                lk = rng.integers(0, 6, size=n).astype(np.uint8)
                lt = rng.integers(0, 4100, size=n).astype(np.uint16)
                lnm = (rng.random(n) < 0.1).astype(U8) if n == 255 else None
                want = check_probe(j, build, lk, lt, ineq, left, lnm, what=n)
                assert want[0].shape[0] == n if left else n < 255 or 0 < want[0].shape[0] < n


# ------------------------------------------------------------------------------------------------------------------------------
# f. past the launch cap
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def past_the_cap():
    cap = _num_cus() * 8 * 256                                            # chgpu_grid_for: at most num_cus * 8 workgroups of 256
    n = cap + 257
    rng = np.random.Generator(np.random.PCG64(930))
    keys = rng.integers(0, 2**64, size=66, dtype=np.uint64)               # 64 present keys spread over all eight key bytes, 2 absent
    assert np.unique(keys).shape[0] == 66
    build = []
    for rows in (n, 1000):
        build.append((keys[rng.integers(0, 64, size=rows)], rng.integers(-2**62, 2**62, size=rows, dtype=np.int64), None, None))
    lk = keys[rng.integers(0, 66, size=n)]
    lt = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
    return cap, build, lk, lt


@pytest.mark.parametrize("ineq,left", [(GE, False), (LT, True)], ids=[">= INNER", "< LEFT"])
def test_past_the_launch_cap(ch, ctx, past_the_cap, ineq, left):
    cap, build, lk, lt = past_the_cap
    assert build[0][0].shape[0] == lk.shape[0] == cap + 257
    want = check_probe(make_join(ch, ctx, build, ineq, left), build, lk, lt, ineq, left)
    tail = np.zeros(lk.shape[0], dtype=bool)
    tail[want[0][want[1] >= 0]] = True                                    # the left rows with a partner
    assert tail[cap:].any() and not tail[cap:].all() and (want[1] == 1).any() and (want[2][want[1] == 0] >= cap).any()


# ------------------------------------------------------------------------------------------------------------------------------
# g. the C entry points with a context
# ------------------------------------------------------------------------------------------------------------------------------
class RawJoin:
    """chgpu_asof_* through the library itself, column handles in, row ids out"""

    def __init__(self, ch, ctx, kind, ineq, key_dt=np.uint32, asof_dt=np.int32):
        self.K, self.ch, self.ctx, self.h = ch._capi, ch, ctx, C.c_void_p()
        self.K.check(self.K.lib().chgpu_asof_create(ctx._h, ch.columns.TAG_OF[np.dtype(key_dt)], ch.columns.TAG_OF[np.dtype(asof_dt)], kind, ineq, C.byref(self.h)))

    def add_block(self, keys, t, nm=None, jm=None):
        """-> (return code, block index)"""
        cols = [self.ctx.upload(x) if x is not None else None for x in (keys, t, nm, jm)]
        bi = C.c_uint64(99)
        rc = self.K.lib().chgpu_asof_add_block(self.h, *[c._h if c is not None else None for c in cols], C.byref(bi))
        return rc, int(bi.value)

    def probe(self, lk, lt, nm=None, with_filter=True):
        """-> (return code, row ids, filter or None, n_out)"""
        cols = [self.ctx.upload(x) if x is not None else None for x in (lk, lt, nm)]
        fh, rh, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        rc = self.K.lib().chgpu_asof_probe(self.h, *[c._h if c is not None else None for c in cols], C.byref(fh) if with_filter else None, C.byref(rh), C.byref(n))
        if rc != self.K.OK:
            assert not fh.value and not rh.value
            return rc, None, None, 0
        filt = self.ch.Column(self.ctx, fh).numpy() if with_filter else None
        return rc, self.ch.Column(self.ctx, rh).numpy(), filt, int(n.value)

    def total_rows(self):
        n = C.c_uint64(0)
        self.K.check(self.K.lib().chgpu_asof_total_rows(self.h, C.byref(n)))
        return int(n.value)

    def close(self):
        assert self.K.lib().chgpu_asof_free(self.h) == self.K.OK


def raw_pairs(rid, filt, left):
    miss = rid == np.uint64(0xFFFFFFFFFFFFFFFF)
    l = np.arange(rid.shape[0], dtype=np.int64) if left else np.flatnonzero(filt).astype(np.int64)
    return l, np.where(miss, -1, (rid >> np.uint64(32)).astype(np.int64)), np.where(miss, -1, (rid & np.uint64(0xFFFFFFFF)).astype(np.int64))


def raw_case(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    blocks = [(rng.integers(0, 4, size=n).astype(np.uint32), rng.integers(-300, 300, size=n).astype(np.int32), None, None) for n in (90, 60)]
    return blocks, rng.integers(0, 5, size=300).astype(np.uint32), rng.integers(-310, 310, size=300).astype(np.int32)


def test_left_probe_without_a_filter(ch, ctx):
    build, lk, lt = raw_case(940)
    for ineq in INEQS:
        j = RawJoin(ch, ctx, ch.JOIN_LEFT, ineq)
        assert [j.add_block(*blk) for blk in build] == [(0, 0), (0, 1)]
        rc, rid, filt, n = j.probe(lk, lt, with_filter=False)
        assert rc == 0 and filt is None and n == 300
        rc2, rid2, filt2, n2 = j.probe(lk, lt, with_filter=True)
        assert rc2 == 0 and n2 == 300 and np.array_equal(rid, rid2)
        assert np.array_equal(filt2, (rid2 != np.uint64(0xFFFFFFFFFFFFFFFF)).astype(U8)) and 0 < filt2.sum() < 300
        want = R.asof_ref(build, lk, lt, ineq, None, True)
        d = R.first_difference(raw_pairs(rid, None, True), want)
        assert d is None, (ineq, d)
        j.close()


ADD_ERRORS = {   # what a bad add_block is given: (keys, asof, null_map, join_mask) made from the good block -> error
    "key type": (lambda k, t: (k.astype(np.uint64), t, None, None), "ERR_BAD_ARGUMENTS"),
    "asof type": (lambda k, t: (k, t.astype(np.uint32), None, None), "ERR_BAD_ARGUMENTS"),
    "asof length": (lambda k, t: (k, t[:-1], None, None), "ERR_SIZES_MISMATCH"),
    "null map length": (lambda k, t: (k, t, np.zeros(k.shape[0] + 1, dtype=U8), None), "ERR_SIZES_MISMATCH"),
    "join mask length": (lambda k, t: (k, t, None, np.ones(k.shape[0] - 1, dtype=U8)), "ERR_SIZES_MISMATCH"),
    "null map type": (lambda k, t: (k, t, np.zeros(k.shape[0], dtype=np.uint16), None), "ERR_SIZES_MISMATCH"),
    "join mask type": (lambda k, t: (k, t, None, np.ones(k.shape[0], dtype=np.int8)), "ERR_SIZES_MISMATCH"),
}
PROBE_ERRORS = {  # (keys, asof, null_map, with_filter) -> error
    "key type": (lambda k, t: (k.astype(np.int32), t, None, True), "ERR_BAD_ARGUMENTS"),
    "asof type": (lambda k, t: (k, t.astype(np.float32), None, True), "ERR_BAD_ARGUMENTS"),
    "asof length": (lambda k, t: (k, t[1:], None, True), "ERR_SIZES_MISMATCH"),
    "null map length": (lambda k, t: (k, t, np.zeros(k.shape[0] - 1, dtype=U8), True), "ERR_SIZES_MISMATCH"),
    "null map type": (lambda k, t: (k, t, np.zeros(k.shape[0], dtype=np.uint32), True), "ERR_SIZES_MISMATCH"),
    "no filter": (lambda k, t: (k, t, None, False), "ERR_BAD_ARGUMENTS"),       # INNER only
}


@pytest.mark.parametrize("left", [False, True], ids=["INNER", "LEFT"])
def test_argument_errors_leave_the_handle_usable(ch, ctx, left):
    K = ch._capi
    build, lk, lt = raw_case(950)
    kind = ch.JOIN_LEFT if left else ch.JOIN_INNER
    want = R.asof_ref(build, lk, lt, GE, None, left)
    assert 0 < (want[1] >= 0).sum() < 300

    def finish(j):
        # the error took no block index and sorted nothing: the handle adds the second block and answers
        assert j.add_block(*build[1]) == (0, 1) and j.total_rows() == 150
        rc, rid, filt, n = j.probe(lk, lt)
        assert rc == 0 and n == want[0].shape[0]
        d = R.first_difference(raw_pairs(rid, filt, left), want)
        assert d is None, d
        j.close()

    for name, (bad, code) in ADD_ERRORS.items():
        j = RawJoin(ch, ctx, kind, GE)
        assert j.add_block(*build[0]) == (0, 0)
        rc, bi = j.add_block(*bad(*build[0][:2]))
        assert rc == getattr(K, code) and bi == 99, (name, rc)
        with pytest.raises(K.ChgpuError):
            K.check(rc)
        finish(j)
    for name, (bad, code) in PROBE_ERRORS.items():
        if name == "no filter" and left:
            continue
        j = RawJoin(ch, ctx, kind, GE)
        assert j.add_block(*build[0]) == (0, 0)
        k, t, nm, with_filter = bad(lk, lt)
        rc = j.probe(k, t, nm, with_filter)[0]
        assert rc == getattr(K, code), (name, rc)
        with pytest.raises(K.ChgpuError) as e:
            K.check(rc)
        assert e.value.code == rc and (name != "no filter" or "filter_u8" in str(e.value))
        finish(j)
