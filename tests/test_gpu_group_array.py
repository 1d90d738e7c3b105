"""groupArray(x) / groupArray(N)(x) under GROUP BY on the device (clickhouse_amd/csrc/group_array_kernels.hip) against
tests/group_array_ref.py.

Every array is compared to the reference bit for bit (group_array_ref.check_column_array, vectorised; the device's row order is free).
Where a case claims a path (the number of radix passes, trimmed arrays, segments reused from an earlier call) it reads the `debug`
option's `group_array plan=` lines, so that it cannot pass by another route."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import group_array_ref as R  # noqa: E402
from group_array_ref import GA_TILE, GA_UNIT, GroupArrayRef, bits  # noqa: E402

pytestmark = pytest.mark.gpu

KEY_DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
VALUE_DTYPES = R.DTYPES


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
    got = [ln[len("chgpu: group_array "):] for ln in err.splitlines() if ln.startswith("chgpu: group_array plan=")]
    return [_ints(dict(kv.split("=", 1) for kv in ln.split() if "=" in kv)) for ln in got]


class Pair:
    """an operator and its reference, fed together"""

    def __init__(self, ch, ctx, kd, vd, max_size=0):
        self.op = ch.GroupArray(kd, vd, max_size=max_size, ctx=ctx)
        self.ref = GroupArrayRef(kd, vd, max_size)

    def close(self):
        self.op.close()

    def add(self, capfd, keys, values, **kw):
        """add_block on both -> the call's plan line, checked against the reference's count"""
        before = len(self.ref)
        capfd.readouterr()
        self.op.add_block(keys, values, **kw)
        plans = _plans(capfd.readouterr().err)
        assert len(plans) == 1 and plans[0]["plan"] == "add", plans
        self.ref.add(keys, values, **kw)
        row_end = kw.get("row_end")
        n = (len(values) if row_end is None else row_end) - kw.get("row_begin", 0)
        assert plans[0]["n"] == n and plans[0]["entered"] == len(self.ref) - before and plans[0]["held"] == (before, len(self.ref)) and plans[0]["rc"] == 0, plans
        assert len(self.op) == len(self.ref)
        return plans[0]

    def merge(self, capfd, other):
        before = len(self.ref)
        capfd.readouterr()
        self.op.merge(other.op)
        plans = _plans(capfd.readouterr().err)
        self.ref.merge(other.ref)
        assert len(plans) == 1 and plans[0]["plan"] == "merge" and plans[0]["held"] == (before, len(self.ref)), plans
        return plans[0]

    def check(self, capfd):
        """finalize equals the reference array by array; -> the plan line"""
        capfd.readouterr()
        k, off, data = self.op.finalize()
        plans = _plans(capfd.readouterr().err)
        assert len(plans) == 1 and plans[0]["plan"] == "finalize", plans
        plan = plans[0]
        msg = R.check_column_array(k, off, data, self.ref)
        assert msg is None, msg
        if len(self.ref):
            gk = self.ref.finalize()[0]
            assert plan["groups"] == (1 if gk is None else len(gk)) and plan["values"] == len(self.ref)
            assert plan["passes"] == self.ref.passes() and plan["trimmed"] == self.ref.trimmed()
        return plan

    def check_for_keys(self, capfd, keys):
        capfd.readouterr()
        off, data = self.op.arrays_for_keys(keys)
        plans = _plans(capfd.readouterr().err)
        assert len(plans) == 1 and plans[0]["plan"] == "for_keys", plans
        want_off, want_data = self.ref.for_keys(keys)
        assert off.dtype == np.uint64 and np.array_equal(off, want_off)
        assert R.same_bits(data, want_data)
        return plans[0]


def _edges(dtype):
    """the type's extremes; floats: NaNs of two payloads and both signs, +-inf, both zeros, denormals, the largest finite values"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        f = np.finfo(dtype)
        u = np.uint32 if dtype.itemsize == 4 else np.uint64
        nans = np.array([0x7FC00001, 0xFFC12345] if dtype.itemsize == 4 else [0x7FF8000000000001, 0xFFF8000012345678], dtype=u).view(dtype)
        rest = np.array([-np.inf, np.inf, f.min, f.max, f.tiny / 2, -f.tiny / 2, f.smallest_subnormal, -0.0, 0.0, np.nan], dtype=dtype)
        return np.concatenate([nans, rest])
    i = np.iinfo(dtype)
    return np.array([i.min, i.max, i.min, i.max, 0], dtype=dtype)


def _random_values(rng, dtype, n):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, size=n)).astype(dtype)
    i = np.iinfo(dtype)
    return rng.integers(i.min, i.max, size=n, dtype=dtype, endpoint=True)


def _increasing_inside_every_array(off, data):
    """values that are global row numbers ascend strictly inside every array"""
    if len(data) < 2:
        return True
    heads = np.zeros(len(data), dtype=bool)
    heads[off[:-1].astype(np.int64)] = True              # (every array of a keyed operator holds a value)
    return bool(np.all((np.diff(data.astype(np.int64)) > 0) | heads[1:]))


# ---- type matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vd", VALUE_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kd", KEY_DTYPES, ids=lambda d: np.dtype(d).name)
def test_type_matrix(ch, ctx, capfd, kd, vd):
    rng = _rng(500 + np.dtype(vd).num * 31 + np.dtype(kd).num)
    n = 5000
    ki = np.iinfo(kd)
    pool = np.unique(np.concatenate([rng.integers(ki.min, ki.max, size=47, dtype=kd, endpoint=True), np.array([ki.min, ki.max, 0], dtype=kd)]))
    keys = pool[rng.integers(0, len(pool), size=n)]
    values = _random_values(rng, vd, n)
    edges = _edges(vd)
    values[100:100 + len(edges)] = edges              # spread over many groups
    keys[3000:3000 + len(edges)] = ki.min             # and all of them in one group, the one below zero for a signed key
    values[3000:3000 + len(edges)] = edges
    filt = (rng.integers(0, 3, size=n) != 0).astype(np.uint8)
    filt[3000:3000 + len(edges)] = 1
    p = Pair(ch, ctx, kd, vd)
    try:
        p.add(capfd, keys[:2600], values[:2600])                   # the copy
        p.add(capfd, keys, values, row_begin=2600, filter=filt)    # the ranked append
        p.check(capfd)
        k, _, data = p.op.finalize()
        assert k.dtype == np.dtype(kd) and data.dtype == np.dtype(vd) and ki.min in k.tolist()
        p.check_for_keys(capfd, pool[::-1].copy())
    finally:
        p.close()


def test_float_keys_are_not_implemented(ch, ctx):
    for kd in (np.float32, np.float64):
        with pytest.raises(ch.ChgpuError) as e:
            ch.GroupArray(kd, np.int64, ctx=ctx)
        assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED


# ---- append edges -----------------------------------------------------------------------------------------------------------------
def _filter(kind, n):
    if kind == "none":
        return None
    f = np.zeros(n, dtype=np.uint8)
    if kind == "ones":
        f[:] = 1
    elif kind == "alternating":
        f[::2] = 7
    elif kind == "last":
        f[-1] = 1
    elif kind == "first":
        f[0] = 255
    return f


@pytest.mark.parametrize("kind", ["none", "zeros", "ones", "alternating", "last", "first"])
@pytest.mark.parametrize("length", [GA_TILE - 1, GA_TILE, GA_TILE + 1, 1])
def test_append_keeps_row_order_at_the_tile_edges(ch, ctx, capfd, length, kind):
    # three blocks in a row, the second cut to an odd sub-range; values are the global row number
    p = Pair(ch, ctx, np.uint32, np.uint64)
    try:
        row = 0
        for b in range(3):
            keys = ((np.arange(length, dtype=np.uint64) + row) % 7).astype(np.uint32)
            values = np.arange(length, dtype=np.uint64) + row
            row += length
            kw = {"filter": _filter(kind, length)}
            if b == 1 and length > 8:
                kw.update(row_begin=3, row_end=length - 5)
            p.add(capfd, keys, values, **kw)
        p.check(capfd)
        _, off, data = p.op.finalize()
        assert _increasing_inside_every_array(off, data)
        # the store itself is in arrival order
        ek, ev = p.op.export_pairs()
        rk, rv = p.ref.pairs()
        assert np.array_equal(bits(ek), rk) and np.array_equal(ev, rv)
    finally:
        p.close()


# ---- stability across tiles and passes --------------------------------------------------------------------------------------------
BASE = 0x00AB00CD00000000


def _key_set(pattern, rng):
    """(light keys, heavy key) as UInt64 whose varying bytes are exactly the pattern's"""
    if pattern == "byte0":
        ks = np.arange(256, dtype=np.uint64) | np.uint64(0x1122334455667700)
    elif pattern == "bytes01":
        ks = rng.permutation(65536)[:3000].astype(np.uint64) | np.uint64(0x1122334455660000)
    elif pattern == "byte5":
        ks = (np.arange(256, dtype=np.uint64) << np.uint64(40)) | np.uint64(0x7700001122334455)
    elif pattern == "bytes07":
        a = rng.permutation(65536)[:3000].astype(np.uint64)
        ks = (a & np.uint64(0xFF)) | ((a >> np.uint64(8)) << np.uint64(56)) | np.uint64(BASE)
    elif pattern == "all8":
        ks = np.unique(rng.integers(0, 2**64 - 1, size=3000, dtype=np.uint64, endpoint=True))   # a PCG draw: hash-like
    else:
        ks = np.array([0xDEADBEEF00C0FFEE, 0xDEADBEEF00C0FFEE], dtype=np.uint64)
    return ks[1:], ks[0]


PATTERN_BYTES = {"byte0": [0], "bytes01": [0, 1], "byte5": [5], "bytes07": [0, 7], "all8": list(range(8)), "single": []}


@pytest.mark.parametrize("pattern", list(PATTERN_BYTES))
def test_every_pass_is_stable_and_only_varying_bytes_are_passed(ch, ctx, capfd, pattern):
    rng = _rng(77)
    light, heavy = _key_set(pattern, rng)
    n = 40_000
    keys = light[rng.integers(0, len(light), size=n)]
    keys[::3] = heavy                                    # one heavy key interleaved with the light ones
    assert R.varying_bytes(keys) == PATTERN_BYTES[pattern]
    values = np.arange(n, dtype=np.uint64)               # arrival order is visible in the values
    p = Pair(ch, ctx, np.uint64, np.uint64)
    try:
        p.add(capfd, keys[:25_000], values[:25_000])
        p.add(capfd, keys[25_000:], values[25_000:])
        plan = p.check(capfd)
        assert plan["passes"] == len(PATTERN_BYTES[pattern]) and plan["cached"] == 0
        _, off, data = p.op.finalize()
        assert _increasing_inside_every_array(off, data)
    finally:
        p.close()


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("size", [64, 512, GA_TILE])
def test_run_heads_on_lane_zero_step_and_tile_boundaries(ch, ctx, capfd, size, extra):
    # With groups of equal size the run heads of the sorted keys are the multiples of the size whatever order the keys sort into: lane 0
    # of a 64-row step (64), a wave's first step (512), a tile's first row (GA_TILE).  One more row (a key of its own) opens a fourth
    # tile of a single row.
    rng = _rng(900 + size + extra)
    groups = 3 * GA_TILE // size
    n = groups * size + extra
    ids = (rng.permutation(1 << 20)[:groups + 1] + 1).astype(np.uint32)
    i = np.arange(n)
    keys = np.where(i < groups * size, ids[i % groups], ids[groups])   # interleaved in arrival, contiguous once sorted
    values = np.arange(n, dtype=np.uint64)
    p = Pair(ch, ctx, np.uint32, np.uint64)
    try:
        p.add(capfd, keys, values)
        plan = p.check(capfd)
        assert plan["groups"] == groups + extra and plan["values"] == n
        _, off, data = p.op.finalize()
        assert _increasing_inside_every_array(off, data)
        ask = np.concatenate([ids[::-1], np.array([0], dtype=np.uint32)])   # every group (the spare id too), then an absent key
        assert p.check_for_keys(capfd, ask)["cached"] == 1
    finally:
        p.close()


def test_one_mid_size_shape_with_three_varying_bytes(ch, ctx, capfd):
    rng = _rng(5)
    n, groups = 1_200_000, 300_000
    keys = rng.integers(0, groups, size=n, dtype=np.uint64) | np.uint64(BASE)
    values = np.arange(n, dtype=np.uint32)
    filt = (rng.integers(0, 8, size=n) != 0).astype(np.uint8)
    p = Pair(ch, ctx, np.uint64, np.uint32)
    try:
        p.add(capfd, keys, values, filter=filt)
        plan = p.check(capfd)
        assert plan["passes"] == 3 and plan["groups"] > 280_000
    finally:
        p.close()


# ---- max_size ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 40, 10_000])
def test_max_size_takes_the_first_n(ch, ctx, capfd, N):
    rng = _rng(21)
    n = 9000
    keys = rng.integers(0, 200, size=n, dtype=np.uint16)
    keys[:40] = 500                                      # a group of exactly 40 values
    keys[40:2500] = 501                                  # and a long one
    values = rng.standard_normal(n).astype(np.float32)
    p = Pair(ch, ctx, np.uint16, np.float32, max_size=N)
    try:
        p.add(capfd, keys[:4000], values[:4000])
        p.add(capfd, keys, values, row_begin=4000)
        plan = p.check(capfd)
        assert (plan["trimmed"] == 0) == (N == 10_000) and len(p.op) == n      # the store keeps every entered row
        p.check_for_keys(capfd, np.array([501, 7, 9999, 500, 501], dtype=np.uint16))
    finally:
        p.close()


def test_max_size_across_a_merge_and_different_sizes_do_not_merge(ch, ctx, capfd):
    rng = _rng(22)
    keys = rng.integers(0, 50, size=6000, dtype=np.uint32)
    values = np.arange(6000, dtype=np.int64)
    dst, src, other = Pair(ch, ctx, np.uint32, np.int64, 5), Pair(ch, ctx, np.uint32, np.int64, 5), Pair(ch, ctx, np.uint32, np.int64, 6)
    try:
        dst.add(capfd, keys[:100], values[:100])         # most groups hold fewer than 5: the rest comes from src, dst's first
        src.add(capfd, keys[100:], values[100:])
        dst.merge(capfd, src)
        dst.check(capfd)
        arrays = dst.ref.arrays()
        assert all(len(a) <= 5 for a in arrays.values()) and any(a[0] < 100 <= a[-1] for a in arrays.values())
        with pytest.raises(ch.ChgpuError) as e:
            dst.op.merge(other.op)
        assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS
        unlimited = ch.GroupArray(np.uint32, np.int64, ctx=ctx)
        with pytest.raises(ch.ChgpuError) as e:
            unlimited.merge(dst.op)
        assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS
        unlimited.close()
        dst.check(capfd)
    finally:
        for p in (dst, src, other):
            p.close()


# ---- merge / export ---------------------------------------------------------------------------------------------------------------
def test_merge_into_and_of_an_empty_operator_and_export_feeds_a_fresh_one(ch, ctx, capfd):
    rng = _rng(23)
    keys = (rng.integers(0, 300, size=7000, dtype=np.int64) - 150).astype(np.int32)
    values = rng.standard_normal(7000)
    a, b, empty, fresh = (Pair(ch, ctx, np.int32, np.float64) for _ in range(4))
    try:
        b.add(capfd, keys[:3000], values[:3000])
        assert a.merge(capfd, b)["entered"] == 3000      # into an empty operator
        a.check(capfd)
        assert a.merge(capfd, empty)["entered"] == 0     # of an empty operator
        assert a.check(capfd)["cached"] == 1             # which changes nothing, the cache included
        a.add(capfd, keys[3000:], values[3000:], filter=(rng.integers(0, 2, size=4000)).astype(np.uint8), row_begin=0, row_end=0)
        a.add(capfd, keys, values, row_begin=3000)
        b_before = b.op.export_pairs()
        a.merge(capfd, b)                                # b's values behind a's
        a.check(capfd)
        b_after = b.op.export_pairs()
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(b_before, b_after))   # src unchanged
        b.check(capfd)
        ek, ev = a.op.export_pairs()
        assert ek.dtype == np.int32 and np.array_equal(bits(ek), a.ref.pairs()[0]) and R.same_bits(ev, a.ref.pairs()[1])
        fresh.add(capfd, ek, ev)
        want = a.op.finalize()
        got = fresh.op.finalize()
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(want, got))
    finally:
        for p in (a, b, empty, fresh):
            p.close()


# ---- for_keys ---------------------------------------------------------------------------------------------------------------------
def test_for_keys_one_long_array_beside_thousands_of_one_and_none(ch, ctx, capfd):
    rng = _rng(24)
    long_n = 3 * GA_UNIT + 5
    light = np.arange(1000, 4000, dtype=np.uint32)
    keys = np.concatenate([light, np.full(long_n, 77, dtype=np.uint32)])
    order = rng.permutation(len(keys))
    keys = keys[order]
    values = rng.integers(-2**62, 2**62, size=len(keys), dtype=np.int64)
    p = Pair(ch, ctx, np.uint32, np.int64)
    try:
        p.add(capfd, keys, values)
        p.check(capfd)
        absent = np.arange(100_000, 102_000, dtype=np.uint32)
        ask = rng.permutation(np.concatenate([light, absent]))           # an order of its own, arrays of one and of none mixed
        ask = np.concatenate([ask[:2500], [77], ask[2500:], [77, 5, 77]]).astype(np.uint32)   # the long array in the middle, then twice more
        plan = p.check_for_keys(capfd, ask)
        assert plan["cached"] == 1 and plan["groups"] == 3001
        off, data = p.op.arrays_for_keys(np.zeros(0, dtype=np.uint32))   # zero rows asked
        assert len(off) == 0 and len(data) == 0 and data.dtype == np.int64
        p.check_for_keys(capfd, absent[:10])                               # only absent keys: ten empty arrays
    finally:
        p.close()


def test_for_keys_builds_the_segments_itself_and_finalize_reuses_them(ch, ctx, capfd):
    rng = _rng(25)
    keys = rng.integers(0, 1000, size=20_000, dtype=np.uint64)
    values = rng.integers(0, 255, size=20_000, dtype=np.uint8)
    p = Pair(ch, ctx, np.uint64, np.uint8)
    try:
        p.add(capfd, keys, values)
        assert p.check_for_keys(capfd, keys[:50])["cached"] == 0
        assert p.check(capfd)["cached"] == 1
        empty = Pair(ch, ctx, np.uint64, np.uint8)
        empty.check_for_keys(capfd, keys[:5])
        empty.close()
    finally:
        p.close()


# ---- without key ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 10])
def test_without_key_the_array_is_the_store_in_order(ch, ctx, capfd, N):
    rng = _rng(26)
    values = rng.standard_normal(5000)
    values[::11] = np.nan
    p = Pair(ch, ctx, None, np.float64, max_size=N)
    try:
        capfd.readouterr()
        k, off, data = p.op.finalize()                   # the empty operator: one row, the empty array
        assert k is None and off.tolist() == [0] and off.dtype == np.uint64 and len(data) == 0 and data.dtype == np.float64
        p.add(capfd, None, values, filter=(rng.integers(0, 2, size=5000)).astype(np.uint8))
        p.add(capfd, None, values, row_begin=17, row_end=4001)
        plan = p.check(capfd)
        assert plan["groups"] == 1 and plan["passes"] == 0 and plan["trimmed"] == (len(p.ref) - 10 if N else 0)
        with pytest.raises(ch.ChgpuError) as e:
            p.op.arrays_for_keys(np.zeros(3, dtype=np.uint32))
        assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS
    finally:
        p.close()


def test_a_keyed_operator_that_holds_nothing_has_no_rows(ch, ctx, capfd):
    p = Pair(ch, ctx, np.int16, np.int8)
    try:
        k, off, data = p.op.finalize()
        assert len(k) == 0 and k.dtype == np.int16 and len(off) == 0 and len(data) == 0
        p.add(capfd, np.array([1, 2], dtype=np.int16), np.array([1, 2], dtype=np.int8), filter=np.zeros(2, dtype=np.uint8))
        k, off, data = p.op.finalize()
        assert len(k) == 0 and len(off) == 0 and len(data) == 0 and len(p.op) == 0
    finally:
        p.close()


# ---- cache ------------------------------------------------------------------------------------------------------------------------
def test_the_segments_are_kept_until_the_store_changes(ch, ctx, capfd):
    rng = _rng(27)
    keys = rng.integers(0, 3000, size=30_000, dtype=np.uint32)
    values = np.arange(30_000, dtype=np.int32)
    p = Pair(ch, ctx, np.uint32, np.int32)
    try:
        p.add(capfd, keys[:20_000], values[:20_000])
        first = p.check(capfd)
        assert first["cached"] == 0 and first["passes"] == 2
        assert p.check(capfd)["cached"] == 1
        assert p.check_for_keys(capfd, keys[:100])["cached"] == 1
        p.add(capfd, keys, values, row_begin=20_000, filter=np.zeros(30_000, dtype=np.uint8))   # nothing entered: the store did not change
        assert p.check(capfd)["cached"] == 1
        p.add(capfd, keys, values, row_begin=20_000)
        after = p.check(capfd)                           # checked against the reference that holds the new rows
        assert after["cached"] == 0 and after["values"] == 30_000
        assert p.check(capfd)["cached"] == 1
    finally:
        p.close()


# ---- atomicity --------------------------------------------------------------------------------------------------------------------
def _snapshot(op):
    k, v = op.export_pairs()
    return len(op), bits(k).tolist(), bits(v).tolist()


def test_a_refused_allocation_leaves_the_operator_as_it_was(ch, capfd):
    c = ch.Context(0)
    K = ch._capi
    try:
        c.set_option("debug", 1)
        rng = _rng(13)
        keys = rng.integers(0, 2000, size=30_000, dtype=np.uint32)
        values = rng.standard_normal(30_000)
        filt = (rng.integers(0, 4, size=30_000) != 0).astype(np.uint8)
        p, twin, other = Pair(ch, c, np.uint32, np.float64, 7), Pair(ch, c, np.uint32, np.float64, 7), Pair(ch, c, np.uint32, np.float64, 7)
        try:
            for q in (p, twin):
                q.add(capfd, keys[:3000], values[:3000])
            other.add(capfd, keys, values)
            other.add(capfd, keys, values)                               # enough that merging it has to grow the store
            untouched = _snapshot(twin.op)

            def refuse_every_allocation_of(call, at_least, finalize_between=True):
                refused = 0
                for nth in range(1, 40):
                    c.set_option("test_group_array_fail_alloc", nth)
                    capfd.readouterr()
                    try:
                        call()
                        c.set_option("test_group_array_fail_alloc", 0)
                        break
                    except ch.ChgpuError as e:
                        assert e.code == K.ERR_OOM
                        refused += 1
                    c.set_option("test_group_array_fail_alloc", 0)
                    assert _snapshot(p.op) == untouched                  # size and export
                    if finalize_between:
                        p.check(capfd)                                   # and a later finalize
                else:
                    raise AssertionError("the call never went through")
                assert refused >= at_least, refused
                return refused

            # add_block that must grow the store, through the ranked append: tile counts, tile offsets, keys, values
            refuse_every_allocation_of(lambda: p.op.add_block(keys, values, filter=filt), 4)
            p.ref.add(keys, values, filter=filt)
            twin.add(capfd, keys, values, filter=filt)
            untouched = _snapshot(twin.op)
            assert _snapshot(p.op) == untouched
            # merge that must grow it again: keys, values
            refuse_every_allocation_of(lambda: p.op.merge(other.op), 2)
            p.ref.merge(other.ref)
            twin.merge(capfd, other)
            untouched = _snapshot(twin.op)
            # finalize: two passes, tile counts and offsets, group keys, segment starts, lengths, their total, array ends, three results
            # (no finalize between the refusals here: it would build the segments the next attempt is meant to build)
            refuse_every_allocation_of(lambda: p.op.finalize(), 9, finalize_between=False)
            p.check(capfd)
            refuse_every_allocation_of(lambda: p.op.arrays_for_keys(keys[:10]), 3)   # (the segments are cached by now)
            p.check(capfd)
            p.check_for_keys(capfd, keys[:10])
            want, got = twin.op.finalize(), p.op.finalize()
            assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(want, got))
        finally:
            for q in (p, twin, other):
                q.close()
    finally:
        c.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_entry_checks_return_their_codes_and_leave_the_operator_usable(ch, ctx, capfd):
    import ctypes as C
    K = ch._capi
    keys = np.arange(100, dtype=np.uint32)
    values = np.arange(100, dtype=np.int64)
    kcol, vcol = ctx.upload(keys), ctx.upload(values)
    p = Pair(ch, ctx, np.uint32, np.int64)
    nokey = ch.GroupArray(None, np.int64, ctx=ctx)
    other = ch.GroupArray(np.uint32, np.int32, ctx=ctx)

    def code(fn, *a, **kw):
        with pytest.raises(ch.ChgpuError) as e:
            fn(*a, **kw)
        return e.value.code, str(e.value)

    try:
        q = p.op
        q.add_block(kcol, vcol)
        p.ref.add(keys, values)
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
        assert code(q.arrays_for_keys, keys.astype(np.uint64))[0] == K.ERR_BAD_ARGUMENTS
        assert code(nokey.arrays_for_keys, keys)[0] == K.ERR_BAD_ARGUMENTS
        q.add_block(kcol, vcol, row_begin=40, row_end=40)                                                       # an empty range is no error
        h = C.c_void_p()
        L = K.lib()
        assert L.chgpu_group_array_create(ctx._h, 77, K.I64, 0, C.byref(h)) == K.ERR_BAD_ARGUMENTS
        assert L.chgpu_group_array_create(ctx._h, K.U32, 77, 0, C.byref(h)) == K.ERR_BAD_ARGUMENTS
        assert L.chgpu_group_array_create(ctx._h, K.F64, K.I64, 0, C.byref(h)) == K.ERR_NOT_IMPLEMENTED
        # NULL outputs on a live handle
        n = C.c_uint64(0)
        a, b, d = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for rc in (L.chgpu_group_array_size(q._h, None), L.chgpu_group_array_finalize(q._h, None, C.byref(b), C.byref(d), C.byref(n)),
                   L.chgpu_group_array_finalize(q._h, C.byref(a), None, C.byref(d), C.byref(n)), L.chgpu_group_array_finalize(q._h, C.byref(a), C.byref(b), None, C.byref(n)),
                   L.chgpu_group_array_finalize(q._h, C.byref(a), C.byref(b), C.byref(d), None), L.chgpu_group_array_export_pairs(q._h, C.byref(a), C.byref(b), None),
                   L.chgpu_group_array_export_pairs(q._h, None, C.byref(b), C.byref(n)), L.chgpu_group_array_for_keys(q._h, kcol._h, None, C.byref(d)),
                   L.chgpu_group_array_for_keys(q._h, kcol._h, C.byref(b), None), L.chgpu_group_array_for_keys(q._h, None, C.byref(b), C.byref(d)),
                   L.chgpu_group_array_merge(q._h, None), L.chgpu_group_array_create(ctx._h, K.U32, K.I64, 0, None)):
            assert rc == K.ERR_BAD_ARGUMENTS and b"NULL" in L.chgpu_last_error()
        # without key: keys_out may be NULL
        assert L.chgpu_group_array_finalize(nokey._h, None, C.byref(b), C.byref(d), C.byref(n)) == K.OK and n.value == 1
        L.chgpu_col_free(b)
        L.chgpu_col_free(d)
        # nothing above changed the operator
        p.check(capfd)
        assert len(q) == 100
    finally:
        p.close()
        nokey.close()
        other.close()
