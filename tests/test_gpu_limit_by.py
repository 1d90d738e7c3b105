"""DISTINCT / LIMIT n OFFSET m BY on the device (clickhouse_amd/csrc/limit_by_kernels.hip) against tests/limit_by_ref.py.

Every filter is compared to the reference bit for bit, and rows_passed and keys() with it.  Where a case claims a path (the plan, the
number of radix passes, growths) it reads the `debug` option's `limit_by plan=` line, so that it cannot pass by another route."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import keycraft as KC  # noqa: E402
import limit_by_ref as R  # noqa: E402
from limit_by_ref import LB_CAP_MIN, LB_TILE, LimitByRef  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = [(1, 0), (1, 1), (2, 0), (2, 1), (3, 5), (1000, 0)]
T = LB_TILE


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
    out = []
    for ln in err.splitlines():
        if ln.startswith("chgpu: limit_by plan="):
            p = dict(kv.split("=", 1) for kv in ln[len("chgpu: limit_by "):].split())
            out.append({k: v if k == "plan" else tuple(int(x) for x in v.split("->")) if "->" in v else int(v) for k, v in p.items()})
    return out


class Pair:
    """an operator and its reference, fed together"""

    def __init__(self, ch, ctx, dtype, length, offset=0, size_hint=0):
        self.op = ch.LimitBy(dtype, length, offset, size_hint=size_hint, ctx=ctx)
        self.ref = LimitByRef(length, offset)

    def close(self):
        self.op.close()

    def feed(self, capfd, keys, **kw):
        """one block through both; -> the call's plan line"""
        capfd.readouterr()
        filt, passed = self.op.filter_block(keys, **kw)
        plans = _plans(capfd.readouterr().err)
        host_kw = {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in kw.items()}
        want, want_passed = self.ref.filter_block(keys.numpy() if hasattr(keys, "numpy") else keys, **host_kw)
        got = filt.numpy()
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), f"first difference at row {int(np.flatnonzero(got != want)[0])}"
        assert passed == want_passed and self.op.keys() == self.ref.keys()
        assert len(plans) == 1 and plans[0]["rc"] == 0 and plans[0]["passed"] == passed and plans[0]["keys"][1] == self.ref.keys()
        return plans[0]


@pytest.fixture
def pair(ch, ctx):
    made = []

    def make(dtype, length, offset=0, size_hint=0):
        made.append(Pair(ch, ctx, dtype, length, offset, size_hint))
        return made[-1]
    yield make
    for p in made:
        p.close()


# ---- the contract's vectors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,offset,blocks,want", R.VECTORS)
def test_the_two_hand_checked_vectors(ch, ctx, length, offset, blocks, want):
    op = ch.LimitBy(np.uint32, length, offset, ctx=ctx)
    for b, w in zip(blocks, want):
        filt, passed = op.filter_block(np.array(b, dtype=np.uint32))
        assert filt.numpy().tolist() == w and passed == sum(w)
    op.close()


# ---- rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,offset", [(1, 0), (2, 1)])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_row_counts_at_the_wave_and_tile_edges(pair, capfd, n, length, offset):
    rng = _rng(n + length)
    p = pair(np.uint32, length, offset)
    keys = rng.integers(0, 7, size=n).astype(np.uint32)
    plan = p.feed(capfd, keys)
    assert plan["n"] == n and plan["plan"] == ("dead" if n == 0 else "claim" if length + offset == 1 else "rank")
    p.feed(capfd, keys[::-1].copy())
    p.feed(capfd, rng.integers(0, 9, size=n).astype(np.uint32))


@pytest.mark.parametrize("length,offset", [(1, 0), (2, 1), (3, 5)])
def test_equal_keys_straddle_waves_tiles_and_workgroups(pair, capfd, length, offset):
    n = 5 * T
    p = pair(np.uint16, length, offset)
    i = np.arange(n)
    # runs of 700 equal keys (they straddle every 64-row and 1024-row edge), then the same keys interleaved
    p.feed(capfd, (i // 700).astype(np.uint16))
    p.feed(capfd, (i % 11).astype(np.uint16))
    q = pair(np.uint16, length, offset)
    q.feed(capfd, (i % 3).astype(np.uint16))


@pytest.mark.parametrize("length,offset", [(2, 1), (3, 5)])
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("size", [64, 512, 2048])
def test_rank_plan_segment_heads_on_lane_zero_step_and_record_tile_boundaries(pair, capfd, size, extra, length, offset):
    # Every row of a fresh operator's first block is live, and the rank plan sorts the records by slot.  With groups of equal size the
    # segment heads are the multiples of the size whatever order the slots sort into: lane 0 of a 64-record step (64), a wave's first
    # step (512), a record tile's first record (2048).  One more row (a key of its own) opens a fourth tile of a single record.
    rng = _rng(size + extra)
    groups = 3 * 2048 // size
    n = groups * size + extra
    ids = (rng.permutation(1 << 20)[:groups + 1] + 1).astype(np.uint32)
    i = np.arange(n)
    contiguous = ids[i // size]
    interleaved = np.where(i < groups * size, ids[i % groups], ids[groups])
    for keys in (contiguous, interleaved):
        p = pair(np.uint32, length, offset)
        plan = p.feed(capfd, keys)
        assert plan["plan"] == "rank" and plan["live"] == n and plan["passes"] >= 1
        p.feed(capfd, keys[::-1].copy())                # the counters the first block left are carried into the ranks


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64])
@pytest.mark.parametrize("begin,end_cut", [(1, 0), (3, 5), (2, 1), (T + 1, 3)])
def test_unaligned_row_ranges_and_views(ch, ctx, pair, capfd, dtype, begin, end_cut):
    rng = _rng(begin * 10 + end_cut)
    n = 3 * T + 7
    keys = rng.integers(0, 50, size=n).astype(dtype)
    filt = (rng.random(n) < 0.8).astype(np.uint8)
    for length, offset in [(1, 0), (2, 1)]:
        p = pair(dtype, length, offset)
        p.feed(capfd, keys, row_begin=begin, row_end=n - end_cut)
        p.feed(capfd, keys, row_begin=begin, row_end=n - end_cut, filter=filt)
        # a view that starts at an odd element of the column's memory: the kernel's wide loads must not assume alignment
        col = ctx.upload(keys)
        view = col.cut(begin, n - end_cut - begin)
        p.feed(capfd, view)
        p.feed(capfd, view, row_begin=1, row_end=view.size() - 2)


# ---- key types -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.KEY_DTYPES)
def test_every_integer_key_type(pair, capfd, dtype):
    rng = _rng(np.dtype(dtype).itemsize * 3 + (np.dtype(dtype).kind == "i"))
    info = np.iinfo(dtype)
    pool = rng.integers(info.min, info.max, size=40, dtype=dtype, endpoint=True)
    pool[:4] = [0, info.max, info.min, -1 if info.min < 0 else info.max - 1]   # zero, the extremes, all ones
    for length, offset in [(1, 0), (2, 1)]:
        p = pair(dtype, length, offset)
        for _ in range(3):
            keys = pool[rng.integers(0, pool.shape[0], size=2 * T + 37)]
            p.feed(capfd, keys, filter=(rng.random(keys.shape[0]) < 0.9).astype(np.uint8))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint32, np.int64, np.uint64])
@pytest.mark.parametrize("which", ["zero", "ones", "both", "both_among_others"])
def test_key_zero_and_the_all_ones_key(pair, capfd, dtype, which):
    rng = _rng(len(which))
    ones = np.array([-1]).astype(dtype)[0] if np.dtype(dtype).kind == "i" else np.iinfo(dtype).max
    pool = {"zero": [0], "ones": [ones], "both": [0, ones], "both_among_others": [0, ones, 1, 2, 3]}[which]
    pool = np.array(pool, dtype=dtype)
    for length, offset in [(1, 0), (2, 1)]:
        p = pair(dtype, length, offset)
        for _ in range(3):
            p.feed(capfd, pool[rng.integers(0, pool.shape[0], size=T + 5)])
        assert p.op.keys() == pool.shape[0]


def test_float_keys_and_no_key_are_refused_and_a_key_type_mismatch_too(ch, ctx):
    import ctypes as C
    K = ch._capi
    for dt in (np.float32, np.float64):
        with pytest.raises(ch.ChgpuError) as e:
            ch.LimitBy(dt, 1, ctx=ctx)
        assert e.value.code == K.ERR_NOT_IMPLEMENTED
    h = C.c_void_p()
    assert K.lib().chgpu_limit_by_create(ctx._h, -1, 1, 0, 0, C.byref(h)) == K.ERR_NOT_IMPLEMENTED
    assert K.lib().chgpu_limit_by_create(ctx._h, 99, 1, 0, 0, C.byref(h)) == K.ERR_BAD_ARGUMENTS
    op = ch.LimitBy(np.uint32, 1, ctx=ctx)
    for wrong in (np.int32, np.uint64, np.uint8):
        with pytest.raises(ch.ChgpuError) as e:
            op.filter_block(np.zeros(4, dtype=wrong))
        assert e.value.code == K.ERR_BAD_ARGUMENTS
    assert op.keys() == 0
    op.close()


# ---- (length, offset): both bounds crossed from every side by carry + rank ------------------------------------------------------
@pytest.mark.parametrize("length,offset", BOUNDS)
def test_every_side_of_both_bounds_by_carry_and_rank(pair, capfd, length, offset):
    rng = _rng(length * 17 + offset)
    bound = length + offset
    seen = np.repeat(np.arange(bound + 2), 4)    # key k was seen seen[k] times in the earlier blocks ...
    more = np.tile(np.arange(4), bound + 2)      # ... and meets more[k] rows in the last one
    ids = np.arange(seen.shape[0], dtype=np.uint32)
    p = pair(np.uint32, length, offset)
    earlier = rng.permutation(np.repeat(ids, seen))
    half = earlier.shape[0] // 2
    p.feed(capfd, earlier[:half])
    p.feed(capfd, earlier[half:])
    plan = p.feed(capfd, rng.permutation(np.repeat(ids, more)))
    assert plan["plan"] == ("claim" if bound == 1 else "rank")
    assert plan["entered"] == int(more.sum()) and plan["live"] == int(more[seen < bound].sum())


# ---- plans ---------------------------------------------------------------------------------------------------------------------
def test_plan_dead_a_second_identical_block_under_distinct(pair, capfd):
    keys = _rng(1).integers(0, 5000, size=4 * T + 3).astype(np.uint64)
    p = pair(np.uint64, 1, 0)
    assert p.feed(capfd, keys)["plan"] == "claim"
    plan = p.feed(capfd, keys)
    assert plan["plan"] == "dead" and plan["live"] == 0 and plan["passed"] == 0 and plan["entered"] == keys.shape[0] and plan["grown"] == 0


def test_plan_claim_one_key_over_five_tiles_and_all_rows_distinct(pair, capfd):
    p = pair(np.uint64, 1, 0)
    plan = p.feed(capfd, np.full(5 * T, 0xDEADBEEF, dtype=np.uint64))
    assert plan["plan"] == "claim" and plan["live"] == 5 * T and plan["passed"] == 1
    q = pair(np.uint64, 1, 0, size_hint=8 * T)
    keys = _rng(2).permutation(np.arange(1, 5 * T + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    plan = q.feed(capfd, keys)
    assert plan["plan"] == "claim" and plan["passed"] == 5 * T and plan["grown"] == 0
    assert q.feed(capfd, keys[::-1].copy())["plan"] == "dead"


LG_CRAFT = 24  # the crafted-slot cases size the table for 2^23 keys: 2^24 cells, so a home cell has three bytes


@pytest.mark.parametrize("slots,passes", [([0x000105], 0), ([0x000105, 0x000205], 1), ([0x010001, 0x020002], 2), ([0x010101, 0x020202, 0x030303], 3),
                                          ([0x000000, 0xFFFFFF], 3), ([0x33, 0x44], 1), ([0x120033, 0x770033], 1)])
def test_plan_rank_passes_only_over_slot_bytes_that_vary(pair, capfd, slots, passes):
    rng = _rng(passes)
    p = pair(np.uint64, 3, 1, size_hint=1 << (LG_CRAFT - 1))
    pool = KC.keys_at_slots(rng, slots, LG_CRAFT)     # an empty table: every key sits in its home cell
    keys = pool[rng.integers(0, pool.shape[0], size=2 * T + 11)]
    plan = p.feed(capfd, keys)
    assert plan["cap"] == (1 << LG_CRAFT, 1 << LG_CRAFT) and plan["plan"] == "rank" and plan["passes"] == passes
    plan = p.feed(capfd, keys[:9])
    assert plan["plan"] in ("rank", "dead")


def test_plan_rank_with_exactly_one_live_row(pair, capfd):
    p = pair(np.uint32, 2, 0)
    keys = np.tile(np.arange(10, dtype=np.uint32), 300)
    p.feed(capfd, keys)                         # every key is at its bound
    keys[1777] = 4242                           # but one new one
    plan = p.feed(capfd, keys)
    assert plan["plan"] == "rank" and plan["live"] == 1 and plan["passes"] == 0 and plan["passed"] == 1


# ---- WHERE ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,offset", [(1, 0), (2, 1)])
def test_where_filter(ch, ctx, pair, capfd, length, offset):
    rng = _rng(77)
    n = 2 * T + 9
    keys = rng.integers(0, 30, size=n).astype(np.uint32)
    a, b = pair(np.uint32, length, offset), pair(np.uint32, length, offset)
    fa, _ = a.op.filter_block(keys, filter=np.ones(n, dtype=np.uint8))       # all ones == no filter
    fb, _ = b.op.filter_block(keys)
    assert np.array_equal(fa.numpy(), fb.numpy())
    c = pair(np.uint32, length, offset)
    plan = c.feed(capfd, keys, filter=np.zeros(n, dtype=np.uint8))           # all zeros: nothing counted
    assert plan["plan"] == "dead" and plan["entered"] == 0 and c.op.keys() == 0
    c.feed(capfd, keys[:100])
    before = c.op.keys()
    c.feed(capfd, keys, filter=np.zeros(n, dtype=np.uint8))
    assert c.op.keys() == before
    d = pair(np.uint32, 1, 0)                                                # a masked-out first occurrence lets the second one pass
    filt = np.ones(6, dtype=np.uint8)
    filt[0] = 0
    d.feed(capfd, np.array([9, 9, 9, 8, 8, 9], dtype=np.uint32), filter=filt)
    got, passed = d.op.filter_block(np.array([9, 8, 7], dtype=np.uint32), filter=np.array([0, 1, 255], dtype=np.uint8))
    assert got.numpy().tolist() == [0, 0, 1] and passed == 1


# ---- the table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,offset", [(1, 0), (2, 1)])
def test_a_chain_longer_than_a_wave_and_a_chain_that_wraps_the_table_end(pair, capfd, length, offset):
    rng = _rng(5)
    lg = LB_CAP_MIN.bit_length() - 1
    chain = KC.keys_at_slots(rng, [777] * 200, lg)                   # 200 keys with one home cell
    wrap = KC.keys_at_slots(rng, [LB_CAP_MIN - 2] * 9, lg)           # these run over the table's end into its first cells
    pool = np.concatenate([chain, wrap])
    p = pair(np.uint64, length, offset)
    for _ in range(3):
        plan = p.feed(capfd, pool[rng.integers(0, pool.shape[0], size=3 * T + 1)])
        assert plan["cap"] == (LB_CAP_MIN, LB_CAP_MIN) and plan["grown"] == 0
    p.feed(capfd, pool)
    assert p.op.keys() == pool.shape[0]


@pytest.mark.parametrize("length,offset", [(1, 0), (2, 1)])
def test_several_growths_in_one_call(pair, capfd, length, offset):
    p = pair(np.uint64, length, offset)
    keys = _rng(6).permutation(np.arange(20_000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    plan = p.feed(capfd, np.concatenate([keys, keys[:3000]]))
    assert plan["grown"] >= 2 and plan["cap"][0] == LB_CAP_MIN and plan["cap"][1] >= 2 * 2 * 20_000 // 2 and p.op.keys() == 20_000
    assert p.feed(capfd, keys)["grown"] == 0


@pytest.mark.parametrize("length,offset", [(1, 0), (2, 1), (3, 5)])
def test_counters_are_carried_through_a_growth(pair, capfd, length, offset):
    rng = _rng(8)
    p = pair(np.uint32, length, offset)
    old = np.arange(500, dtype=np.uint32)
    p.feed(capfd, old[rng.integers(0, 500, size=1500)])                                  # block 1 counts
    plan = p.feed(capfd, rng.permutation(np.arange(1000, 9000, dtype=np.uint32)))         # block 2 grows
    assert plan["grown"] >= 1 and plan["cap"][1] > plan["cap"][0]
    p.feed(capfd, np.concatenate([old, old, old, old])[rng.permutation(2000)])           # block 3 checks
    p.feed(capfd, np.array([0, 0, 0], dtype=np.uint32))                                   # key 0 lives out of line: its counter moved too


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_contract(ch, ctx):
    import ctypes as C
    K = ch._capi
    L = K.lib()

    def code(fn):
        with pytest.raises(ch.ChgpuError) as e:
            fn()
        return e.value.code

    assert code(lambda: ch.LimitBy(np.uint32, 0, ctx=ctx)) == K.ERR_BAD_ARGUMENTS                     # group_length == 0
    assert code(lambda: ch.LimitBy(np.uint32, 1, 2**32 - 1, ctx=ctx)) == K.ERR_NOT_IMPLEMENTED         # offset + length = 2^32
    assert code(lambda: ch.LimitBy(np.uint32, 2**32, 0, ctx=ctx)) == K.ERR_NOT_IMPLEMENTED
    assert code(lambda: ch.LimitBy(np.uint32, 1, size_hint=2**30 + 1, ctx=ctx)) == K.ERR_TOO_MANY_ROWS  # more keys than a table takes
    for length, offset in [(2**32 - 2, 0), (1, 2**32 - 2), (2**32 - 1, 0)]:                            # the last sums that fit
        op = ch.LimitBy(np.uint8, length, offset, ctx=ctx)
        filt, passed = op.filter_block(np.array([1, 1, 2], dtype=np.uint8))
        assert filt.numpy().tolist() == ([1, 1, 1] if offset == 0 else [0, 0, 0]) and op.keys() == 2
        op.close()
    op = ch.LimitBy(np.uint32, 2, 1, ctx=ctx)
    keys = ctx.upload(np.arange(10, dtype=np.uint32))
    out, n = C.c_void_p(), C.c_uint64(0)
    assert L.chgpu_limit_by_filter_block(op._h, keys._h, 0, 10, None, None, C.byref(n)) == K.ERR_BAD_ARGUMENTS      # NULL outputs
    assert L.chgpu_limit_by_filter_block(op._h, keys._h, 0, 10, None, C.byref(out), None) == K.ERR_BAD_ARGUMENTS
    assert L.chgpu_limit_by_filter_block(op._h, None, 0, 10, None, C.byref(out), C.byref(n)) == K.ERR_BAD_ARGUMENTS
    assert L.chgpu_limit_by_keys(op._h, None) == K.ERR_BAD_ARGUMENTS
    assert code(lambda: op.filter_block(keys, 4, 3)) == K.ERR_BAD_ARGUMENTS                            # row_begin > row_end
    assert code(lambda: op.filter_block(keys, 0, 11)) == K.ERR_BAD_ARGUMENTS                           # a range past the column
    assert code(lambda: op.filter_block(keys, filter=np.ones(9, dtype=np.uint8))) == K.ERR_SIZES_MISMATCH
    assert code(lambda: op.filter_block(keys, 2, 5, filter=np.ones(3, dtype=np.uint8))) == K.ERR_SIZES_MISMATCH
    assert code(lambda: op.filter_block(keys, filter=np.ones(10, dtype=np.uint32))) == K.ERR_BAD_ARGUMENTS
    assert op.keys() == 0
    filt, passed = op.filter_block(keys, 7, 7)                                                         # an empty range is no error
    assert filt.size() == 0 and passed == 0
    op.close()
    # 2^32 rows in one call: refused before anything is read (the column is allocated, never written)
    op = ch.LimitBy(np.uint8, 1, ctx=ctx)
    huge = ctx.alloc(np.uint8, 2**32)
    assert code(lambda: op.filter_block(huge)) == K.ERR_TOO_MANY_ROWS
    huge.free()
    ctx.trim()
    op.close()


@pytest.mark.parametrize("length,offset", [(1, 0), (2, 1)])
def test_a_refused_allocation_leaves_every_counter_as_it_was(ch, ctx, capfd, length, offset):
    rng = _rng(12)
    first = rng.integers(0, 300, size=900).astype(np.uint32)
    second = np.concatenate([rng.permutation(np.arange(100, 6100, dtype=np.uint32)), first[:500]])
    failed_at = []
    for nth in range(1, 64):
        p = Pair(ch, ctx, np.uint32, length, offset)
        try:
            p.feed(capfd, first)
            keys_before = p.op.keys()
            ctx.set_option("test_limit_by_fail_alloc", nth)
            refused = None
            try:
                capfd.readouterr()
                p.op.filter_block(second)
            except ch.ChgpuError as e:
                refused = e
            finally:
                ctx.set_option("test_limit_by_fail_alloc", 0)
            if refused is None:
                break   # the call makes fewer than nth allocations: it went through (and is checked no further)
            assert refused.code == ch._capi.ERR_OOM and "test_limit_by_fail_alloc" in str(refused)
            plans = _plans(capfd.readouterr().err)
            assert len(plans) == 1 and plans[0]["rc"] == ch._capi.ERR_OOM and plans[0]["keys"] == (keys_before, keys_before)
            failed_at.append(nth)
            assert p.op.keys() == keys_before           # nothing of the failed call was counted
            p.feed(capfd, second)                       # the same block succeeds and equals a reference that never saw the failure
            p.feed(capfd, np.concatenate([first, second]))
        finally:
            p.close()
    assert len(failed_at) >= 8 and failed_at == list(range(1, len(failed_at) + 1))   # every allocation of a growing call was refused once


# ---- determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,offset", [(1, 0), (2, 1), (3, 5)])
def test_the_same_input_gives_the_same_filters_for_every_launch_geometry(ch, ctx, length, offset):
    rng = _rng(21)
    blocks = [rng.integers(0, 3000, size=n).astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F) for n in (4 * T + 5, 6 * T, 3 * T - 1)]
    runs = []
    for grid in (0, 0, 1, 3):
        ctx.set_option("test_limit_by_grid", grid)
        try:
            op = ch.LimitBy(np.uint64, length, offset, ctx=ctx)
            runs.append([op.filter_block(b) for b in blocks])
            runs[-1] = [(f.numpy(), n) for f, n in runs[-1]] + [op.keys()]
            op.close()
        finally:
            ctx.set_option("test_limit_by_grid", 0)
    ref = LimitByRef(length, offset)
    want = [ref.filter_block(b) for b in blocks]
    for r in runs:
        assert r[-1] == ref.keys()
        for (gf, gn), (wf, wn) in zip(r[:-1], want):
            assert np.array_equal(gf, wf) and gn == wn


# ---- helpers and shim ----------------------------------------------------------------------------------------------------------
def _rows_of(cols):
    return list(zip(*[c if isinstance(c, list) else c.tolist() for c in cols]))


def _host(col):
    return col.to_list() if hasattr(col, "to_list") else col.numpy() if hasattr(col, "numpy") else col


def _expect_block(seen, rows, key_pos, length, offset):
    out = []
    for r in rows:
        k = tuple(r[p] for p in key_pos)
        c = seen.get(k, 0)
        if c < offset + length:
            seen[k] = c + 1
            if c >= offset:
                out.append(r)
    return out


@pytest.mark.parametrize("shape", ["packed", "keydict", "string"])
def test_distinct_block_over_two_blocks(ch, ctx, shape):
    rng = _rng(31)
    op = ch.BlockKeys(ctx=ctx)
    seen = {}
    for blk in range(2):
        n = 3000
        if shape == "packed":
            host = [rng.integers(0, 40 + 25 * blk, size=n).astype(np.uint32), rng.integers(0, 5, size=n).astype(np.uint16)]
            cols = list(host)
        elif shape == "keydict":
            host = [rng.integers(0, 9 + 4 * blk, size=n).astype(np.uint64) << np.uint64(40), rng.integers(0, 7, size=n).astype(np.uint64),
                    rng.integers(0, 3, size=n).astype(np.uint32)]
            cols = list(host)
        else:
            words = [b"", b"a", b"ab", b"abc" * 30, b"b", b"zebra"] + [b"w%d" % i for i in range(blk * 20, blk * 20 + 60)]
            vals = [words[int(i)] for i in rng.integers(0, len(words), size=n)]
            host = [vals, rng.integers(0, 2, size=n).astype(np.uint8)]
            cols = [ch.ColumnString.from_values(ctx, vals), host[1]]
        want = _expect_block(seen, _rows_of(host), list(range(len(host))), 1, 0)
        got = ch.distinct_block(op, cols)
        assert got is not None and _rows_of([_host(c) for c in got]) == want
    assert ch.distinct_block(op, cols) is None            # the same block again: no survivor
    op.close()


def test_limit_by_block_passes_a_full_chunk_through_and_keeps_non_key_columns(ch, ctx):
    op = ch.BlockKeys(length=2, offset=0, ctx=ctx)
    a = np.array([1, 2, 1, 2, 3], dtype=np.int64)
    payload = np.arange(5, dtype=np.float64)
    cols = [a, payload]
    assert ch.limit_by_block(op, [0], cols) is cols       # every row passes: the chunk as it came
    got = ch.limit_by_block(op, [0], [np.array([1, 3, 3, 4], dtype=np.int64), np.array([10., 11., 12., 13.])])
    assert got[0].numpy().tolist() == [3, 4] and got[1].numpy().tolist() == [11., 13.]
    op.close()


def test_shim_transforms_against_host_loops(tmp_path):
    exe = tmp_path / "limit_by_shim_driver"
    lib_dir = os.path.join(REPO, "clickhouse_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", os.path.join(REPO, "tests", "limit_by_shim_driver.cpp"), "-L" + lib_dir, "-lchgpu", "-lpthread",
                        "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "limit_by_shim_driver OK" in r.stdout, r.stdout + r.stderr
