"""The folding merges on the device (Replacing, Collapsing, Summing / Aggregating) against tests/merge_fold_ref.py, bit for bit.

T is the fold tile.  The shapes are the smallest at which each mechanism can break: group lengths around the wave and the tile, a group
that crosses whole tiles with no head in them, heads and tails exactly on tile edges, every row its own group, one group for the whole
input, 0 and 1 rows, 1 / 2 / 3 / 257 runs and a group whose rows come from every run; keys that are equal only as order words (-0.0 / +0.0,
NaN), a second key column that splits a group on a tile edge, descending keys, every key dtype.  Every case is checked against the
vectorised reference, inputs of up to 200 rows also against the per-row one (test_merge_fold_ref.py holds the two together)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_fold_ref as F  # noqa: E402
import merge_sorted_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ASC = [(0, False, 1)]
KINDS3 = ["sum", "max", "min"]


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    return ch.Context(0)


@pytest.fixture(scope="module")
def T():
    from clickhouse_amd import merge_fold
    return merge_fold.TILE


def layout(lens, n_runs, rng=None):
    """Groups of the given lengths in merged order, dealt to n_runs sorted runs.  rng None: a group's rows go to the runs in blocks (run
    numbers never decrease along the group, so the merged order is the order written here, and a group of n_runs rows or more has a row
    from every run); else at random.  -> (key column over the concatenation, offsets, order) where a column written in merged order is
    column[order] over the concatenation."""
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    key = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    if rng is None:
        within = np.arange(n) - np.repeat(np.cumsum(lens) - lens, lens)
        run = within * n_runs // np.repeat(lens, lens)
    else:
        run = rng.integers(0, n_runs, n)
    order = np.argsort(run, kind="stable")
    return key[order], R.offsets_of(np.bincount(run, minlength=n_runs)), order


def extents(T):
    return [[1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 1, 2], [T, T, 5], [T - 1, 1, T, 1], [3, 3 * T, 3 * T - 3, 9], [1] * (T + 3), [2 * T + 7], [1], []]


def check_replacing(ch, ctx, keys, spec, offs, version=None, is_deleted=None, cleanup=False):
    d = R.describe(keys, spec)
    want = F.replacing_vector(d, version, is_deleted, cleanup)
    if len(keys[0]) <= 200:
        assert np.array_equal(F.replacing_cursor(d, offs, version, is_deleted, cleanup), want)
    got = ch.replacing_merge_rows([ctx.upload(k) for k in keys], spec, offs, version, is_deleted, cleanup).numpy()
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), (got[:8], want[:8])
    return got


def check_collapsing(ch, ctx, keys, spec, offs, sign):
    d = R.describe(keys, spec)
    want = F.collapsing_vector(d, sign)
    if len(keys[0]) <= 200:
        assert np.array_equal(F.collapsing_cursor(d, offs, sign), want)
    got = ch.collapsing_merge_rows([ctx.upload(k) for k in keys], spec, offs, sign).numpy()
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), (got[:8], want[:8])
    return got


def check_folding(ch, ctx, keys, spec, offs, values, kinds, drop_zero=False):
    d = R.describe(keys, spec)
    want = F.folding_vector(d, values, kinds, drop_zero)
    if len(keys[0]) <= 200:
        cur = F.folding_cursor(d, offs, values, kinds, drop_zero)
        assert np.array_equal(cur[0], want[0]) and np.array_equal(cur[1], want[1]) and all(np.array_equal(a, b) for a, b in zip(cur[2], want[2]))
    first, last, results = ch.aggregating_merge_rows([ctx.upload(k) for k in keys], spec, offs, values, kinds, drop_zero=drop_zero)
    first, last = first.numpy(), last.numpy()
    assert first.dtype == np.uint64 and np.array_equal(first, want[0]), (first[:8], want[0][:8])
    assert last.dtype == np.uint64 and np.array_equal(last, want[1]), (last[:8], want[1][:8])
    assert len(results) == len(values)
    for r, w, v in zip(results, want[2], values):
        r = r.numpy()
        assert r.dtype == v.dtype and np.array_equal(r, w), (r[:8], w[:8])
    return first, last, [r.numpy() for r in results]


def random_args(rng, n):
    version = R.random_column(rng, np.int64, n, 2)
    deleted = rng.integers(0, 2, n).astype(np.uint8)
    sign = np.where(rng.integers(0, 2, n) == 1, 1, -1).astype(np.int8)
    values = [rng.integers(-1, 2, n).astype(np.int8), R.random_column(rng, np.uint64, n, 2), R.random_column(rng, np.int32, n, 3)]
    return version, deleted, sign, values


def check_all(ch, ctx, keys, spec, offs, rng):
    n = len(keys[0])
    version, deleted, sign, values = random_args(rng, n)
    check_replacing(ch, ctx, keys, spec, offs, version, deleted, True)
    check_collapsing(ch, ctx, keys, spec, offs, sign)
    check_folding(ch, ctx, keys, spec, offs, values, KINDS3, True)


@pytest.mark.parametrize("n_runs", [1, 2, 3])
def test_group_extents_around_the_wave_and_the_tile(ch, ctx, T, n_runs):
    rng = np.random.Generator(np.random.PCG64(n_runs))
    for lens in extents(T):
        for dealt in (None, rng):
            key, offs, _ = layout(lens, n_runs, dealt)
            check_all(ch, ctx, [key], ASC, offs, rng)
            check_replacing(ch, ctx, [key], ASC, offs)


def test_257_runs_and_a_group_from_every_run(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(257))
    key, offs, _ = layout([300, 1, 257, T + 40, 2, 600], 257)
    assert np.all(np.diff(offs.astype(np.int64)) > 0)
    check_all(ch, ctx, [key], ASC, offs, rng)
    dev = [ctx.upload(key)]
    sign = np.ones(len(key), dtype=np.int8)
    launches = ctx.counters()["KernelLaunches"]
    ch.collapsing_merge_rows(dev, ASC, offs, sign)
    # the sorted check 2, the sign check 2, the key build and nine rounds of two launches, then heads, tile, carry, count, offsets, emit
    assert ctx.counters()["KernelLaunches"] - launches <= 2 + 2 + (1 + 2 * 9) + 6
    launches = ctx.counters()["KernelLaunches"]
    ch.replacing_merge_rows([ctx.upload(np.sort(key))], ASC, [0, len(key)], check=False)
    assert ctx.counters()["KernelLaunches"] - launches <= 1 + 6      # one run: the pairs of the identity
    key, offs, _ = layout([7] * 500, 257, rng)
    check_all(ch, ctx, [key], ASC, offs, rng)


def test_more_tiles_than_threads_of_the_one_workgroup_kernels(ch, ctx, T):
    """2 * 256 * T + T + 5 rows in two runs: 514 tiles, so k_fold_carry's threads own up to three tiles each and k_fold_offsets scans the
    tile counts in three passes of 256 with a carry between them.  Seeded group lengths of 1 .. 9, and one group from seven positions
    before the end of tile 255 to eleven positions into tile 257 (it covers tile 256 whole and crosses the edge between the passes)."""
    rng = np.random.Generator(np.random.PCG64(514))
    total, start, long = 2 * 256 * T + T + 5, 256 * T - 7, T + 18

    def short(n):
        lens = rng.integers(1, 10, n)              # more than enough: cut where the sum reaches n, the last one shortened to fit
        ends = np.cumsum(lens)
        k = int(np.searchsorted(ends, n))
        lens[k] -= ends[k] - n
        return lens[:k + 1]

    lens = np.concatenate([short(start), [long], short(total - start - long)])
    assert lens.sum() == total and lens.min() >= 1
    first = np.cumsum(lens) - lens
    g = int(np.flatnonzero(lens == long)[0])
    assert first[g] // T == 255 and (first[g] + long - 1) // T == 257
    key, offs, _ = layout(lens, 2, rng)
    assert len(key) == total
    sign = np.where(rng.integers(0, 2, total) == 1, 1, -1).astype(np.int8)
    got = check_collapsing(ch, ctx, [key], ASC, offs, sign)
    assert len(got) > 256 * T // 9                  # outputs in every pass of the offsets
    values = [rng.integers(-1, 2, total).astype(np.int8), R.random_column(rng, np.uint64, total, 2)]
    d = R.describe([key], ASC)
    want = F.folding_vector(d, values, ["sum", "sum"], True)
    first_rows, last_rows, results = ch.summing_merge_rows([ctx.upload(key)], ASC, offs, values)
    assert np.array_equal(first_rows.numpy(), want[0]) and np.array_equal(last_rows.numpy(), want[1])
    for r, w, v in zip(results, want[2], values):
        assert r.numpy().dtype == v.dtype and np.array_equal(r.numpy(), w)


def test_zeros_and_nans_of_different_runs_share_a_group(ch, ctx):
    rng = np.random.Generator(np.random.PCG64(5))
    for dtype in (np.float64, np.float32):
        key = np.array([-0.0, np.nan, 0.0, np.nan, -0.0, 0.0, np.nan], dtype=dtype)
        offs = R.offsets_of([2, 2, 3])
        got = check_replacing(ch, ctx, [key], ASC, offs)
        assert got.tolist() == [5, 6]
        assert check_collapsing(ch, ctx, [key], ASC, offs, np.array([-1, 1, 1, -1, -1, 1, 1], dtype=np.int8)).tolist() == [0, 5, 6]
        first, last, (total,) = check_folding(ch, ctx, [key], ASC, offs, [np.arange(7, dtype=np.uint16)], ["sum"])
        assert first.tolist() == [0, 1] and last.tolist() == [5, 6] and total.tolist() == [0 + 2 + 4 + 5, 1 + 3 + 6]
        key = np.array([np.nan, -0.0, np.nan, 0.0], dtype=dtype)       # NaN first
        assert check_replacing(ch, ctx, [key], [(0, False, -1)], R.offsets_of([2, 2])).tolist() == [2, 3]
        cols, offs = R.sort_runs([R.random_column(rng, dtype, 700)], [(0, True, 1)], R.offsets_of([100, 0, 350, 250])), R.offsets_of([100, 0, 350, 250])
        check_all(ch, ctx, cols, [(0, True, 1)], offs, rng)


def test_a_second_key_splits_a_group_on_a_tile_edge(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(6))
    for lens in ([T - 3, 3, 5, T + 1], [T, T], [2 * T - 1, 1, 1]):
        second, offs, _ = layout(lens, 2)
        first = np.zeros(len(second), dtype=np.uint32)                # every first word ties: the heads come from the gathered column
        spec = [(0, False, 1), (1, False, 1)]
        check_all(ch, ctx, [first, second.astype(np.int16)], spec, offs, rng)
        got = check_replacing(ch, ctx, [first, second.astype(np.int16)], spec, offs)
        assert len(got) == len(lens)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_key_dtype_in_both_directions(ch, ctx, T, dtype):
    rng = np.random.Generator(np.random.PCG64(70 + R.DTYPES.index(dtype)))
    lens = [300, 0, 500, T + 9]
    for desc in (False, True):
        spec = [(0, desc, 1), (1, not desc, 1)]
        offs = R.offsets_of(lens)
        cols = R.sort_runs([R.random_column(rng, dtype, int(offs[-1]), 5), R.random_column(rng, np.int16, int(offs[-1]), 1)], spec, offs)
        check_all(ch, ctx, cols, spec, offs, rng)
    one = [(0, True, 1)]                                               # a single key column: one-byte keys take the sort chain
    cols = R.sort_runs([R.random_column(rng, dtype, int(offs[-1]), 5)], one, offs)
    check_all(ch, ctx, cols, one, offs, rng)


def test_empty_and_single_row_inputs(ch, ctx):
    for n in (0, 1):
        key = np.arange(n, dtype=np.int64)
        for offs in ([0, n], [0, 0, n, n]):
            check_replacing(ch, ctx, [key], ASC, offs, key.astype(np.uint8), np.zeros(n, dtype=np.uint8), True)
            check_collapsing(ch, ctx, [key], ASC, offs, np.ones(n, dtype=np.int8))
            first, _, results = check_folding(ch, ctx, [key], ASC, offs, [key.astype(np.int8), key.astype(np.uint64)], ["sum", "min"])
            assert len(first) == n and [len(r) for r in results] == [n, n]
            check_folding(ch, ctx, [key], ASC, offs, [], [])


# ---------------------------------------------------------------------------------------------
# Replacing
# ---------------------------------------------------------------------------------------------
def test_replacing_version_ties_prefer_the_later_row(ch, ctx):
    key = np.zeros(4, dtype=np.int64)
    assert check_replacing(ch, ctx, [key], ASC, [0, 2, 4], np.array([3, 3, 3, 1], dtype=np.uint8)).tolist() == [2]     # across runs: the later run
    assert check_replacing(ch, ctx, [key], ASC, [0, 4], np.array([1, 3, 3, 2], dtype=np.uint32)).tolist() == [2]       # inside a run
    assert check_replacing(ch, ctx, [key], ASC, [0, 1, 2, 3, 4], np.array([1, 3, 3, 2], dtype=np.int16)).tolist() == [2]
    assert check_replacing(ch, ctx, [key], ASC, [0, 2, 4], np.array([-1, -1, -2, -1], dtype=np.int8)).tolist() == [3]
    assert check_replacing(ch, ctx, [key], ASC, [0, 2, 4]).tolist() == [3]                                              # no version: the last row


def test_replacing_greatest_version_anywhere_in_a_long_group(ch, ctx, T):
    lens = [3 * T + 5, 4]
    key, offs, order = layout(lens, 3)
    n = len(key)
    for at in (0, 5, T, 3 * T + 4):            # first in the group, early in another tile than the tail, on a tile edge, last
        merged = np.ones(n, dtype=np.int64)
        merged[at] = 7
        got = check_replacing(ch, ctx, [key], ASC, offs, merged[order])
        assert len(got) == 2 and merged[order][got[0]] == 7


def test_replacing_versions_at_the_type_extremes(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(8))
    key, offs, _ = layout([5, T + 1, 64, 2 * T], 3, rng)
    n = len(key)
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    check_replacing(ch, ctx, [key], ASC, offs, np.array([lo, -1, 0, hi], dtype=np.int64)[rng.integers(0, 4, n)])
    check_replacing(ch, ctx, [key], ASC, offs, np.array([lo, lo + 1], dtype=np.int64)[rng.integers(0, 2, n)])
    check_replacing(ch, ctx, [key], ASC, offs, np.array([0, 2**63 - 1, 2**63, 2**64 - 1], dtype=np.uint64)[rng.integers(0, 4, n)])
    check_replacing(ch, ctx, [key], ASC, offs, np.array([-128, 127, 0], dtype=np.int8)[rng.integers(0, 3, n)])


def test_replacing_is_deleted_and_cleanup(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(9))
    key, offs, _ = layout([3, T, 1, 1, T + 7, 2], 2, rng)
    n = len(key)
    version = rng.integers(0, 3, n).astype(np.uint16)
    deleted = rng.integers(0, 2, n).astype(np.uint8)
    kept = check_replacing(ch, ctx, [key], ASC, offs, version, deleted, False)
    cleaned = check_replacing(ch, ctx, [key], ASC, offs, version, deleted, True)
    assert len(kept) == 6 and np.array_equal(cleaned, kept[deleted[kept] == 0])
    assert len(check_replacing(ch, ctx, [key], ASC, offs, version, np.ones(n, dtype=np.uint8), True)) == 0       # every group is cleaned away
    assert len(check_replacing(ch, ctx, [key], ASC, offs, version, np.ones(n, dtype=np.uint8), False)) == 6
    bad = deleted.copy()
    bad[[T + 900, 17, 2 * T + 3]] = [2, 2, 255]
    for cleanup in (False, True):
        with pytest.raises(ch.ChgpuError) as e:
            ch.replacing_merge_rows([ctx.upload(key)], ASC, offs, version, bad, cleanup)
        assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS and "row 17 " in str(e.value)


# ---------------------------------------------------------------------------------------------
# Collapsing
# ---------------------------------------------------------------------------------------------
def outcome_signs(length):
    """the five outcomes for a group of `length` rows (even, >= 4) in merged order, and the rows each emits"""
    alt = np.tile(np.array([-1, 1], dtype=np.int8), length // 2)
    more_positive = alt.copy()
    more_positive[0] = 1                        # cp = cn + 2
    one_more_negative = np.concatenate([alt[:-1], [-1]]).astype(np.int8)[1:]      # + .. - -: cp + 1 = cn, length - 1 rows
    return [(alt, 2), (-alt, 0), (np.concatenate([alt, [1]]).astype(np.int8), 1), (one_more_negative, 1), (more_positive, 1)]


@pytest.mark.parametrize("long_groups", [False, True])
def test_collapsing_outcomes(ch, ctx, T, long_groups):
    cases = outcome_signs(3 * T + 6 if long_groups else 4)
    lens = [len(s) for s, _ in cases]
    for n_runs in (1, 3):
        key, offs, order = layout(lens, n_runs)
        merged = np.concatenate([s for s, _ in cases])
        sign = merged[order]
        got = check_collapsing(ch, ctx, [key], ASC, offs, sign)
        assert np.bincount(key[got], minlength=5).tolist() == [c for _, c in cases]
        assert sign[got].tolist() == [-1, 1, 1, -1, 1]


def test_collapsing_every_group_cancels(ch, ctx, T):
    key, offs, order = layout([2] * (T + 10), 2)
    merged = np.tile(np.array([1, -1], dtype=np.int8), T + 10)      # cp = cn, the last row negative
    assert len(check_collapsing(ch, ctx, [key], ASC, offs, merged[order])) == 0


def test_collapsing_two_row_outputs_around_a_tile_edge(ch, ctx, T):
    for lead in (0, 1, 3):                      # the pairs begin on an even position, on an odd one (a pair straddles every tile edge), ..
        lens = ([lead] if lead else []) + [2] * (T + 10)
        key, offs, order = layout(lens, 2)
        merged = np.concatenate([np.ones(lead, dtype=np.int8), np.tile(np.array([-1, 1], dtype=np.int8), T + 10)])
        got = check_collapsing(ch, ctx, [key], ASC, offs, merged[order])
        assert len(got) == (1 if lead else 0) + 2 * (T + 10)        # every pair emits both rows: more than T outputs from one tile


def test_collapsing_bad_signs_name_the_lowest_row(ch, ctx, T):
    key, offs, _ = layout([3, T, T + 7], 2)
    for value in (0, 2):
        sign = np.ones(len(key), dtype=np.int8)
        sign[[2 * T + 1, 31, T + 5]] = value
        with pytest.raises(ch.ChgpuError) as e:
            ch.collapsing_merge_rows([ctx.upload(key)], ASC, offs, sign)
        assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS and "row 31 " in str(e.value)


# ---------------------------------------------------------------------------------------------
# Folding
# ---------------------------------------------------------------------------------------------
def test_folding_sums_wrap_in_the_column_type(ch, ctx, T):
    key, offs, _ = layout([2, T + 1, 300], 2)
    n = len(key)
    _, _, (a, b) = check_folding(ch, ctx, [key], ASC, offs, [np.full(n, 127, dtype=np.int8), np.full(n, 2**64 - 1, dtype=np.uint64)], ["sum", "sum"])
    assert a.tolist() == [((127 * length + 128) % 256) - 128 for length in (2, T + 1, 300)] and a[0] == -2
    assert b.tolist() == [2**64 - 2, 2**64 - (T + 1), 2**64 - 300]


def test_folding_drop_zero_needs_every_sum_to_be_zero(ch, ctx):
    key = np.array([1, 1, 2, 2, 3, 3, 4], dtype=np.int64)
    a = np.array([5, -5, 5, -5, 1, 1, 0], dtype=np.int16)
    b = np.array([0, 0, 1, 0, 0, 0, 0], dtype=np.uint8)
    m = np.array([9, 9, 9, 9, 9, 9, 9], dtype=np.int32)
    for offs in ([0, 7], [0, 3, 7]):
        first, _, _ = check_folding(ch, ctx, [key], ASC, offs, [a, b, m], ["sum", "sum", "max"], True)
        assert key[first].tolist() == [2, 3]                         # group 1 and group 4 sum to 0 in all SUM columns; group 2 only in one
        first, _, _ = check_folding(ch, ctx, [key], ASC, offs, [a, b, m], ["sum", "sum", "max"], False)
        assert key[first].tolist() == [1, 2, 3, 4]
        first, _, _ = check_folding(ch, ctx, [key], ASC, offs, [], [], True)      # no value columns: nothing is dropped
        assert key[first].tolist() == [1, 2, 3, 4]


def test_folding_min_max_at_the_type_extremes(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(12))
    key, offs, _ = layout([1, 65, T + 3, 2 * T], 3, rng)
    n = len(key)
    for dtype in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64):
        info = np.iinfo(dtype)
        v = np.array([info.min, info.max, 0, 1], dtype=dtype)[rng.integers(0, 4, n)]
        w = np.array([info.min, info.min + 1], dtype=dtype)[rng.integers(0, 2, n)]
        x = np.array([info.max, info.max - 1], dtype=dtype)[rng.integers(0, 2, n)]
        check_folding(ch, ctx, [key], ASC, offs, [v, v, w, x, x, w], ["min", "max", "max", "min", "max", "min"])


def test_folding_mixed_widths_and_kinds(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(13))
    key, offs, _ = layout([1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5], 3, rng)
    n = len(key)
    values = [R.random_column(rng, np.uint8, n), R.random_column(rng, np.int64, n, 3), R.random_column(rng, np.uint32, n, 9)]
    for kinds in (["max", "sum", "min"], ["sum", "min", "sum"]):
        for drop_zero in (False, True):
            check_folding(ch, ctx, [key], ASC, offs, values, kinds, drop_zero)
    eight = [R.random_column(rng, dt, n, 2) for dt in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64)]
    check_folding(ch, ctx, [key], ASC, offs, eight, ["sum", "min", "max", "sum", "min", "max", "sum", "min"], True)
    check_folding(ch, ctx, [key], ASC, offs, [], [])


# ---------------------------------------------------------------------------------------------
# Blocks
# ---------------------------------------------------------------------------------------------
def _blocks(T, seed):
    """three sorted blocks of (key Int32 descending, payload UInt64, version UInt16, is_deleted UInt8, sign Int8, a Int8, b UInt64)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    spec = [(0, True, 1)]
    blocks = []
    for n in (T + 5, 0, 700):
        key = R.random_column(rng, np.int32, n, 30)
        cols = [key, rng.integers(0, 2**63, n).astype(np.uint64), rng.integers(0, 3, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8),
                np.where(rng.integers(0, 2, n) == 1, 1, -1).astype(np.int8), rng.integers(-1, 2, n).astype(np.int8), R.random_column(rng, np.uint64, n, 2)]
        blocks.append(R.sort_runs(cols, spec, R.offsets_of([n])))
    glued = [np.concatenate([b[k] for b in blocks]) for k in range(7)]
    return blocks, glued, spec, R.offsets_of([len(b[0]) for b in blocks])


def test_block_functions(ch, ctx, T):
    blocks, glued, spec, offs = _blocks(T, 21)
    d = R.describe(glued, spec)
    dev = [[ctx.upload(c) for c in b] for b in blocks]
    cols, rows = ch.replacing_merge(dev, spec, version=2, is_deleted=3, cleanup=True)
    want = F.replacing_vector(d, glued[2], glued[3], True)
    assert np.array_equal(rows.numpy(), want) and all(np.array_equal(c.numpy(), g[want.astype(np.int64)]) for c, g in zip(cols, glued))
    cols, rows = ch.collapsing_merge(dev, spec, sign=4)
    want = F.collapsing_vector(d, glued[4])
    assert np.array_equal(rows.numpy(), want) and all(np.array_equal(c.numpy(), g[want.astype(np.int64)]) for c, g in zip(cols, glued))
    first, _, (p, a, b) = F.folding_vector(d, [glued[1], glued[5], glued[6]], ["sum"] * 3, True)
    cols, rows = ch.summing_merge([[blk[0], blk[1], blk[5], blk[6]] for blk in dev], spec)      # None: every integer column that is no key
    got = [c.numpy() for c in cols]
    assert np.array_equal(rows.numpy(), first) and np.array_equal(got[0], glued[0][first.astype(np.int64)])
    assert np.array_equal(got[1], p) and np.array_equal(got[2], a) and np.array_equal(got[3], b)
    first, _, (a, b) = F.folding_vector(d, [glued[5], glued[6]], ["sum", "sum"], True)
    cols, rows = ch.summing_merge([[blk[0], blk[1], blk[5], blk[6]] for blk in dev], spec, columns_to_sum=[2, 3])
    got = [c.numpy() for c in cols]
    i = first.astype(np.int64)
    assert np.array_equal(rows.numpy(), first) and np.array_equal(got[0], glued[0][i]) and np.array_equal(got[1], glued[1][i])
    assert np.array_equal(got[2], a) and np.array_equal(got[3], b)
    first, last, (mx, sm) = F.folding_vector(d, [glued[2], glued[5]], ["max", "sum"], False)
    cols, rows = ch.aggregating_merge(dev, spec, {2: "max", 5: "sum", 1: "anyLast", 3: "any"})
    got = [c.numpy() for c in cols]
    i, j = first.astype(np.int64), last.astype(np.int64)
    assert np.array_equal(rows.numpy(), first) and np.array_equal(got[2], mx) and np.array_equal(got[5], sm)
    assert np.array_equal(got[0], glued[0][i]) and np.array_equal(got[1], glued[1][j]) and np.array_equal(got[3], glued[3][i])
    assert np.array_equal(got[4], glued[4][i]) and np.array_equal(got[6], glued[6][i])


def test_unsorted_runs_are_refused_and_float_values_too(ch, ctx):
    key = np.array([1, 3, 2, 4], dtype=np.int64)
    sign = np.ones(4, dtype=np.int8)
    dev = [ctx.upload(key)]
    for call in (lambda: ch.collapsing_merge_rows(dev, ASC, [0, 4], sign), lambda: ch.replacing_merge_rows(dev, ASC, [0, 4]),
                 lambda: ch.summing_merge_rows(dev, ASC, [0, 4], [sign])):
        with pytest.raises(ch.ChgpuError) as e:
            call()
        assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS and "row 2 " in str(e.value)
    assert ch.collapsing_merge_rows(dev, ASC, [0, 2, 4], sign).numpy().tolist() == [0, 2, 1, 3]
    with pytest.raises(TypeError):
        ch.summing_merge_rows(dev, ASC, [0, 4], [np.zeros(4)])
